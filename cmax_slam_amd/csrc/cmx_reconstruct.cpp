// cmx_reconstruct.cpp -- cmx_backend_recon_*: the panorama of ALL events warped along the FINAL trajectory, for a spline of any knot
// count.  One call of recon_add* is the vote loop of EventWarper::computeImageOfWarpedEvents (event_pano_warper.cpp:188-196,
// :233-311) over exactly the events handed in, added into a plane that belongs to the reconstruction alone: no old / new split, no
// alpha, no IG, no blur, and nothing of the window state, the resident evaluation point, the map or the exchange sets is touched.
// On top of it, the whole-trajectory contrast and its gradient with respect to a left increment of EVERY control pose
// (recon_contrast, recon_grad_add*, recon_grad_get, recon_eval_from): the image pass over the plane and a second pass over the same
// events, in the adjoint form of the window path -- per batch one 3-vector through the 3 x 3N spline Jacobian,
// so nothing grows with the knot count but the 2 x 3K sums.  And for an optimiser that evaluates the SAME events many times: events
// bound once (recon_bind_from), evaluated through a batch-pose table, a tile sort of the reconstruction's own and LDS votes
// (recon_eval_bound).  And for the online case -- a settled head, a free tail: the batches under fixed knots voted once
// into a base plane (recon_freeze_head), and the evaluation side of the native bundle adjustment (recon_solve_*, driven by
// cmx_solver.cpp's FR-CG machine).  And for a recording that grows: the spline lengthened (recon_extend), events appended
// to the binding (recon_bind_append_from), the freeze line moved forward (recon_advance_head) and the settled events' memory given
// back (recon_release_head) -- book-keeping around the same kernels over sub-ranges.
// Kernels: cmx_recon.hip.
#include <limits>

#include "cmx_context.hpp"

// Raw events per internal slice (a whole number of batches).  Staging -- two slots of pinned + device memory for the packed events
// and the batch times -- is bounded by this, not by the length of the input; at 2048 packed events per workgroup a full slice is
// 2048 workgroups, eight per compute unit.
constexpr int64_t kSliceEvents = 1 << 22;
// A slice holds at most max(slice size, one batch) packed events, and the vote kernel indexes a slice with ints: both are
// kept at or below 2^30, far from the wrap.
constexpr int kMaxSliceEvents = 1 << 30;
static std::atomic<int64_t> g_slice_events{kSliceEvents};
int recon_diag_slice_events(int n) {  // CMX_DIAG_RECON_SLICE_EVENTS: small inputs through the multi-slice path (tests)
  if (n < 0 || n > kMaxSliceEvents) return CMX_ERR_INVALID_ARG;
  g_slice_events.store(n > 0 ? (int64_t)n : kSliceEvents, std::memory_order_relaxed);
  return CMX_OK;
}

struct ReconSlot {
  uint32_t *h_xy = nullptr, *d_xy = nullptr;
  long long *h_bt = nullptr, *d_bt = nullptr;
  size_t xy_cap = 0, bt_cap = 0, h_bt_cap = 0;  // (h_bt: host paths only)
  hipEvent_t up = nullptr, done = nullptr;  // upload complete (copy stream) / vote kernel complete (context stream)
  bool busy = false;
};

// Output staging of the per-event export (cmx_backend_recon_warp*, host output): the kernel of slice k writes into d_*, a copy on the
// download stream moves it into pinned h_*, and the host pool copies it into the caller's arrays while slice k+1 runs.
struct ReconWarpSlot {
  void *d_xy = nullptr, *h_xy = nullptr;
  unsigned char *d_fl = nullptr, *h_fl = nullptr;
  size_t cap = 0;                            // events (16 bytes of coordinates each, the wider format)
  hipEvent_t kdone = nullptr, down = nullptr;  // kernel complete (context stream) / download complete (download stream)
};

// Events bound to the reconstruction (cmx_backend_recon_bind_from): the sampled events of the range in time order, their batch
// times, and what the tile-sorted vote pass of cmx_backend_recon_eval_bound needs -- all of it the reconstruction's own, a TileSort
// beside the context's (cmx_ctx::sort, bin_valid, ...), which is not used: the window's sort survives a whole-trajectory evaluation.
// Resident bytes per sampled event: 4 (xy) + 4 (keys) + 4 (sxy) + 4 (sbatch) = 16, plus 80 per batch (time, PoseR); the counting
// sort's histogram table and the chunk table depend on the panorama, not on the events.
struct ReconBound {
  int64_t n_events = 0;                 // events of the bound range
  BatchPlan plan;                       // its batches; plan.n_packed = events the sampling selects
  uint32_t *d_xy = nullptr;             // [n_packed] packed, time order, per_batch slots per batch
  long long *d_bt = nullptr;            // [nb] batch pose times
  PoseR *d_poseR = nullptr;             // [nb] batch poses of the current evaluation
  TileSort ts;                          // the events in tile order, the chunk table; ts.d_fallback: votes of the last evaluation that left their LDS window
  // the table's allocation and every vote launch's size: an upper bound known on the host (workgroups beyond the table's true
  // length return at once; launching that length instead was measured and gained nothing: 0.453 -> 0.452 ms at 20M events);
  // events per full chunk
  int max_chunks = 0, chunk_events = 0;
  unsigned long long *h_stat = nullptr; // pinned: [0] = n_inside, [1] = fallback word of the last evaluation
  bool sorted = false;
  int64_t sorts = 0;
  double fallback_frac = 0;
  // ---- a binding that grows (bind_append_from, release_head).  n_events, plan and every batch / packed index above
  // count from the bind; d_xy, d_bt and d_poseR start at packed event base_sampled / batch base_batches: packed event i is
  // d_xy[i - base_sampled], batch b is d_bt[b - base_batches].  rel_* are what release_head has given back (base_* <= rel_*: the
  // entries between them are dead space until the live ones move, see release_head) -- neither to be confused with the frozen
  // head's counts, which say where the active events start, not where the arrays do.
  size_t xy_cap = 0, bt_cap = 0;        // elements of d_xy, and of d_bt and d_poseR
  int64_t rel_batches = 0, rel_sampled = 0, rel_events = 0;
  int64_t base_batches = 0, base_sampled = 0;  // batch / packed event at element 0 of the arrays: at most the released counts
  // the raw events of the open tail [open_tail_from(n_events), n_events), as the store held them: what the next append cuts again
  uint32_t *d_tail_xy = nullptr;
  int64_t *d_tail_t = nullptr;
  size_t tail_cap = 0;
  int64_t tail_n = 0;
  long long t_last = 0;                 // time of the last bound event (n_events > 0)
  uint32_t *xy_at(int64_t i) const { return d_xy + (i - base_sampled); }
  long long *bt_at(int b) const { return d_bt + (b - base_batches); }
  PoseR *pose_at(int b) const { return d_poseR + (b - base_batches); }
  int64_t resident_sampled() const { return plan.n_packed - rel_sampled; }
  void release() {
    void *dev[] = {d_xy, d_bt, d_poseR, d_tail_xy, d_tail_t};
    for (void *p : dev) (void)hipFree(p);
    ts.release();
    if (h_stat) (void)hipHostFree(h_stat);
    *this = ReconBound{};
  }
};

// A frozen head of the binding (cmx_backend_recon_freeze_head): the batches [0, b_act) whose pose only the first
// num_fixed knots can move (frozen_prefix, cmx_ingest.hpp), voted ONCE at the knots of the freeze into a base plane of the
// reconstruction's own -- fp32 in default mode, the 2^-30 fixed-point plane in deterministic mode -- with the count of its voting
// events beside it.  An evaluation of the binding then starts from the base and walks the active batches [b_act, nb) alone: their
// events, a tile sort of their own in the binding's TileSort, a chunk table at the chunk rule of their count.
struct ReconFrozen {
  int num_fixed = 0;                      // 0: no frozen head
  int b_act = 0;                          // first active batch
  int64_t sampled = 0;                    // sampled events of the frozen batches
  unsigned long long inside = 0;          // ... of which voted
  void *d_base = nullptr;                 // [Wp * Hp] float, or fix_t in deterministic mode
  unsigned long long *d_inside = nullptr; // `inside` on the device, what an evaluation's counter starts from
  std::vector<double> knots;              // the first num_fixed knots as they were at the freeze (x, y, z, w)
  int max_chunks = 0, chunk_events = 0;   // the active part's chunk table (plan_chunks of its count)
  void release() {
    (void)hipFree(d_base);
    (void)hipFree(d_inside);
    *this = ReconFrozen{};
  }
};

// What cmx_backend_recon_solve keeps between its trial points: the start knots, pinned staging for the moved knots, and host memory
// the device writes an evaluation's results into (contrast and mean, the two counters, the free gradient entries).
struct ReconSolve {
  std::vector<double> k0, last_x;
  int num_fixed = 0, measure = CMX_VARIANCE;
  double sigma = 1.0;
  double *h_knots = nullptr;              // pinned [K][4]
  double *h_cm = nullptr;                 // pinned: contrast, mu
  unsigned long long *h_cnt = nullptr;    // pinned: n_inside, n_voted
  double *h_grad = nullptr, *d_grad = nullptr;  // mapped [3K]
  bool have_last = false;
  int64_t evals = 0, waits = 0;           // of the last solve: evaluations, and host waits inside them
  void release() {
    void *host[] = {h_knots, h_cm, h_cnt, h_grad};
    for (void *p : host)
      if (p) (void)hipHostFree(p);
    *this = ReconSolve{};
  }
};

struct ReconState {
  KnotSupport sup;
  int B = 0, rate = 0, per_batch = 0;
  bool deterministic = false;
  double blend[kMaxOrder * kMaxOrder] = {0};
  Quat *d_knots = nullptr;
  double *d_delta = nullptr;
  float *d_plane = nullptr;               // the plane (default mode), or the fp32 view of d_fixed made by get / render
  unsigned long long *d_fixed = nullptr;  // deterministic mode: 2^-30 fixed-point votes
  unsigned long long *d_inside = nullptr;
  long long *d_err = nullptr;             // error words of the device-side batch-time pass (event store)
  int64_t n_sampled = 0;
  hipStream_t copy_stream = nullptr;      // uploads of slice i+1 beside the vote kernel of slice i
  ReconSlot slot[2];
  hipStream_t down_stream = nullptr;      // per-event export: downloads of slice i beside the kernel of slice i+1 (created at first use)
  ReconWarpSlot wslot[2];
  // ---- contrast and gradient (all of it the reconstruction's own: the context's blur state and image buffers are not touched)
  double sigma_built = -1.0;              // sigma the taps / G^T 1 factors below were built for (-1: none)
  int radius = 0;
  float taps[2 * kMaxRadius + 1] = {1.f};
  float *d_cx = nullptr, *d_cy = nullptr; // G^T 1 = cx(x) cy(y), Wp and Hp floats
  unsigned char *d_tflags = nullptr;      // tile occupancy of the plane (launch_tile_flags)
  unsigned *d_tile_list = nullptr, *d_tile_count = nullptr;  // large panoramas: the image passes' work list, in tile order
  double *d_partials = nullptr;           // [2][tiles] moment rows of the image pass
  double *d_cm = nullptr;                 // contrast, mu (recon_moments_finalize)
  float *d_jt = nullptr;                  // Jt = G^T (G plane), allocated at the first want_grad
  double *d_gsum = nullptr;               // [2][3K]: S1, S2, allocated at the first want_grad
  unsigned long long *d_voted = nullptr;  // events that passed the vote test in the gradient pass
  double *d_rows = nullptr;               // deterministic mode: one row of window sums per gather workgroup of a slice ...
  int *d_row_win = nullptr;               // ... and the rows' first knots
  size_t rows_cap = 0;                    // (workgroups)
  bool grad_open = false;                 // a gradient pass is open: recon_contrast(want_grad) ran and nothing voted since
  int64_t g_sampled = 0;                  // events the gradient pass has sampled
  int measure = CMX_VARIANCE;
  double mu = 0;
  // ---- bound events (recon_bind_from .. recon_unbind): survive restart, dropped by begin and end
  bool bound = false;
  ReconBound bnd;
  ReconFrozen frozen;                     // of the binding: dropped with it, and by restart
  int g_num_fixed = 0;                    // the open gradient pass is a frozen evaluation's: grad[0, 3 g_num_fixed) is zero by definition
  ReconSolve solve;
  uint32_t *d_app_xy = nullptr;           // bind_append_from's scratch stream, "open tail ++ new range": raw events ...
  int64_t *d_app_t = nullptr;             // ... and their times, count + B of them at most
  size_t app_cap = 0;
  int64_t host_waits = 0;                // times a host thread has waited for the device in this reconstruction's calls
};
// every place one of these calls blocks on the stream goes through here (cmx_backend_recon_solve reports the count per evaluation)
static hipError_t recon_wait(cmx_ctx *c, ReconState *r) {
  r->host_waits++;
  return hipStreamSynchronize(c->stream);
}
// the binding changes, goes, or the knots are set anew: no frozen head any more, and the next evaluation sorts all events again
static void frozen_drop(cmx_ctx *c, ReconState *r) {
  if (!r->frozen.num_fixed && !r->frozen.d_base) return;
  (void)hipStreamSynchronize(c->stream);  // (an evaluation queued earlier may still read the base)
  r->frozen.release();
  r->bnd.sorted = false;
  r->g_num_fixed = 0;
}

void recon_release(cmx_ctx *c) {
  ReconState *r = c ? c->recon : nullptr;
  if (!r) return;
  (void)hipSetDevice(c->device);
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  if (r->copy_stream) { (void)hipStreamSynchronize(r->copy_stream); (void)hipStreamDestroy(r->copy_stream); }
  for (ReconSlot &s : r->slot) {
    if (s.h_xy) (void)hipHostFree(s.h_xy);
    if (s.h_bt) (void)hipHostFree(s.h_bt);
    (void)hipFree(s.d_xy);
    (void)hipFree(s.d_bt);
    if (s.up) (void)hipEventDestroy(s.up);
    if (s.done) (void)hipEventDestroy(s.done);
  }
  if (r->down_stream) { (void)hipStreamSynchronize(r->down_stream); (void)hipStreamDestroy(r->down_stream); }
  for (ReconWarpSlot &s : r->wslot) {
    if (s.h_xy) (void)hipHostFree(s.h_xy);
    if (s.h_fl) (void)hipHostFree(s.h_fl);
    (void)hipFree(s.d_xy);
    (void)hipFree(s.d_fl);
    if (s.kdone) (void)hipEventDestroy(s.kdone);
    if (s.down) (void)hipEventDestroy(s.down);
  }
  void *dev[] = {r->d_knots, r->d_delta, r->d_plane, r->d_fixed, r->d_inside, r->d_err, r->d_cx, r->d_cy, r->d_tflags, r->d_tile_list,
                 r->d_tile_count, r->d_partials, r->d_cm, r->d_jt, r->d_gsum, r->d_voted, r->d_rows, r->d_row_win, r->d_app_xy, r->d_app_t};
  for (void *p : dev) (void)hipFree(p);
  r->bnd.release();
  r->frozen.release();
  r->solve.release();
  delete r;
  c->recon = nullptr;
}

// common front door: a plain back-end context (a group's handle has no reconstruction: CMX_ERR_STATE), bound to its device
static int recon_enter(cmx_ctx *c, bool need_begun) {
  if (!c || c->kind != KIND_BE) return fail(c, CMX_ERR_STATE, "not a back-end context");
  if (c->group) return fail(c, CMX_ERR_STATE, "reconstruction is not available on a group handle");
  if (need_begun && !c->recon) return fail(c, CMX_ERR_STATE, "cmx_backend_recon_begin has not succeeded");
  return bind_device(c);
}

// knot values for the trajectory of begin (begin itself, restart, eval_bound); plane, counters and gradient state start over.
// Nothing is allocated or freed.
// (knots_xyzw == NULL, eval_bound only: the current knots stay, and nothing of the caller's is read -- no wait)
// from_base (eval_bound with a frozen head): plane and counters start from the frozen batches' votes instead of zero.
// staged (cmx_backend_recon_solve): the knots are in pinned memory that stays untouched until the evaluation's own wait -- none here.
static int recon_start_over(cmx_ctx *c, ReconState *r, const double *knots_xyzw, bool from_base = false, bool staged = false) {
  const size_t np = (size_t)c->Wp * c->Hp;
  const ReconFrozen &fz = r->frozen;
  const bool base = from_base && fz.num_fixed > 0;
  r->grad_open = false;
  r->g_num_fixed = 0;
  r->n_sampled = base ? fz.sampled : 0;
  if (knots_xyzw) {
    static_assert(sizeof(Quat) == 4 * sizeof(double), "knots travel as (x, y, z, w) doubles");
    HIP_TRY(c, hipMemcpyAsync(r->d_knots, knots_xyzw, (size_t)r->sup.K * sizeof(Quat), hipMemcpyHostToDevice, c->stream));
    launch_recon_delta(r->d_knots, r->sup.K, r->d_delta, c->stream);
  }
  if (base) {  // the base restore: one device-to-device copy in the plane's own format, and the counter's start value
    if (r->d_fixed) {
      HIP_TRY(c, hipMemsetAsync(r->d_plane, 0, np * sizeof(float), c->stream));
      HIP_TRY(c, hipMemcpyAsync(r->d_fixed, fz.d_base, np * sizeof(unsigned long long), hipMemcpyDeviceToDevice, c->stream));
    } else {
      HIP_TRY(c, hipMemcpyAsync(r->d_plane, fz.d_base, np * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
    }
    HIP_TRY(c, hipMemcpyAsync(r->d_inside, fz.d_inside, sizeof(unsigned long long), hipMemcpyDeviceToDevice, c->stream));
  } else {
    HIP_TRY(c, hipMemsetAsync(r->d_plane, 0, np * sizeof(float), c->stream));
    HIP_TRY(c, hipMemsetAsync(r->d_inside, 0, sizeof(unsigned long long), c->stream));
    if (r->d_fixed) HIP_TRY(c, hipMemsetAsync(r->d_fixed, 0, np * sizeof(unsigned long long), c->stream));
  }
  HIP_TRY(c, hipGetLastError());
  if (knots_xyzw && !staged) HIP_TRY(c, recon_wait(c, r));  // the caller's knot array is free again
  return CMX_OK;
}

static int recon_begin_inner(cmx_ctx *c, int order, int K, const double *knots_xyzw, int64_t start_ns, int64_t dt_ns, int B, int rate) {
  ReconState *r = new ReconState();
  c->recon = r;
  r->sup = KnotSupport{order, K, (long long)start_ns, (long long)dt_ns};
  r->B = B; r->rate = rate;
  r->per_batch = (B + rate - 1) / rate;
  r->deterministic = c->deterministic;
  blending_matrix(order, r->blend);
  const size_t np = (size_t)c->Wp * c->Hp;
  HIP_TRY(c, hipStreamCreateWithFlags(&r->copy_stream, hipStreamNonBlocking));
  for (ReconSlot &s : r->slot) {
    HIP_TRY(c, hipEventCreateWithFlags(&s.up, hipEventDisableTiming));
    HIP_TRY(c, hipEventCreateWithFlags(&s.done, hipEventDisableTiming));
  }
  HIP_TRY(c, hipMalloc((void **)&r->d_knots, (size_t)K * sizeof(Quat)));
  HIP_TRY(c, hipMalloc((void **)&r->d_delta, (size_t)(K - 1) * 3 * sizeof(double)));
  HIP_TRY(c, hipMalloc((void **)&r->d_plane, np * sizeof(float)));
  HIP_TRY(c, hipMalloc((void **)&r->d_inside, sizeof(unsigned long long)));
  HIP_TRY(c, hipMalloc((void **)&r->d_err, 2 * sizeof(long long)));
  if (r->deterministic) HIP_TRY(c, hipMalloc((void **)&r->d_fixed, np * sizeof(unsigned long long)));
  return recon_start_over(c, r, knots_xyzw);
}

int cmx_backend_recon_begin(cmx_ctx *c, int order, int K, const double *knots_xyzw, int64_t start_ns, int64_t dt_ns,
                            int event_batch_size, int event_sample_rate) {
  int rc = recon_enter(c, false);
  if (rc) return rc;
  if (order != 2 && order != 4) return fail(c, CMX_ERR_INVALID_ARG, "spline order %d unsupported (2 = linear, 4 = cubic)", order);
  if (K < order || K > (1 << 28)) return fail(c, CMX_ERR_INVALID_ARG, "K=%d outside [%d, 2^28]", K, order);
  if (!knots_xyzw || dt_ns <= 0) return fail(c, CMX_ERR_INVALID_ARG, "bad spline description");
  if (event_batch_size <= 0 || event_sample_rate <= 0) return fail(c, CMX_ERR_INVALID_ARG, "batch size / sample rate must be > 0");
  if (event_batch_size > kMaxSliceEvents) return fail(c, CMX_ERR_INVALID_ARG, "batch size %d above 2^30", event_batch_size);
  recon_release(c);  // a second begin starts over
  rc = recon_begin_inner(c, order, K, knots_xyzw, start_ns, dt_ns, event_batch_size, event_sample_rate);
  if (rc) recon_release(c);
  return rc;
}

int cmx_backend_recon_end(cmx_ctx *c) {
  int rc = recon_enter(c, false);
  if (rc) return rc;
  recon_release(c);  // (nothing to free before a begin: not an error)
  return CMX_OK;
}

// ---- one add: batches of the call (plan_batches), slices of whole batches
static int recon_slice_batches(const ReconState *r) { return slice_batches_of(g_slice_events.load(std::memory_order_relaxed), r->B); }
static int recon_plan(cmx_ctx *c, const ReconState *r, int64_t n, BatchPlan *p, int *slice_batches) {
  if (!plan_batches(n, r->B, r->rate, p)) return fail(c, CMX_ERR_INVALID_ARG, "too many batches");
  *slice_batches = recon_slice_batches(r);
  return CMX_OK;
}

static ReconArgs recon_args(const cmx_ctx *c, const ReconState *r) {
  ReconArgs a{};
  a.cam = be_args(c);
  a.cam.xy = nullptr; a.cam.poseR = nullptr; a.cam.poses = nullptr; a.cam.planes = nullptr;
  a.order = r->sup.order; a.K = r->sup.K;
  a.start_ns = r->sup.start_ns; a.dt_ns = r->sup.dt_ns;
  for (int i = 0; i < kMaxOrder * kMaxOrder; i++) a.blend[i] = r->blend[i];
  a.knots = r->d_knots; a.delta = r->d_delta;
  a.B = r->B;
  a.per_batch = r->per_batch;
  a.run = recon_run(r->per_batch);
  a.plane = r->d_plane;
  a.fixed = r->deterministic ? r->d_fixed : nullptr;
  a.n_inside = r->d_inside;
  return a;
}

// the gradient pass's view of the same launch: the events and the spline of recon_args, Jt and the border factors, the sums
static ReconGatherArgs recon_gather_args(const cmx_ctx *c, const ReconState *r) {
  ReconGatherArgs g{};
  g.ev = recon_args(c, r);
  g.itilde = r->d_jt;
  g.cx = r->d_cx; g.cy = r->d_cy; g.r = r->radius;
  g.gsum = r->d_gsum;
  g.n_voted = r->d_voted;
  return g;
}

// first thing of every pass over events: a vote pass closes an open gradient pass, a gradient pass needs one
static int recon_pass_enter(cmx_ctx *c, ReconState *r, bool grad) {
  if (!grad) { r->grad_open = false; return CMX_OK; }
  if (!r->grad_open) return fail(c, CMX_ERR_STATE, "no gradient pass is open (cmx_backend_recon_contrast with want_grad, and no add since)");
  return CMX_OK;
}

// one slice of the gradient pass; deterministic mode: the workgroups' rows, then their sum in workgroup order
static int queue_gather(cmx_ctx *c, ReconState *r, ReconGatherArgs &g) {
  const int blocks = recon_gather_blocks(g.ev);
  if (blocks <= 0) return CMX_OK;
  if (r->deterministic) {
    if ((size_t)blocks > r->rows_cap) {
      HIP_TRY(c, hipStreamSynchronize(c->stream));  // (an earlier slice may still be reading the rows)
      (void)hipFree(r->d_rows); (void)hipFree(r->d_row_win);
      r->d_rows = nullptr; r->d_row_win = nullptr; r->rows_cap = 0;
      HIP_TRY(c, hipMalloc((void **)&r->d_rows, (size_t)blocks * 2 * 3 * kReconWindow * sizeof(double)));
      HIP_TRY(c, hipMalloc((void **)&r->d_row_win, (size_t)blocks * sizeof(int)));
      r->rows_cap = (size_t)blocks;
    }
    g.rows = r->d_rows;
    g.row_win = r->d_row_win;
  }
  launch_recon_gather(g, c->stream);
  launch_recon_gather_rows(g, blocks, c->stream);
  return CMX_OK;
}
// one slice of a pass over events, as g.ev describes it: its votes, or its share of the gradient sums
static int queue_slice(cmx_ctx *c, ReconState *r, ReconGatherArgs &g, bool grad) {
  if (grad) return queue_gather(c, r, g);
  launch_recon_votes(g.ev, c->stream);
  return CMX_OK;
}

// staging of one slot.  The host paths (pinned) hold packed events and batch times in pinned memory and on the device; the store
// path reads the store's events in place and forms the batch times on the device, so it holds the device table alone.
static int slot_ensure(cmx_ctx *c, ReconSlot &s, size_t n_xy, size_t n_bt, bool pinned) {
  if (n_xy > s.xy_cap) {
    if (s.h_xy) HIP_TRY(c, hipHostFree(s.h_xy));
    s.h_xy = nullptr;
    (void)hipFree(s.d_xy);
    s.d_xy = nullptr;
    s.xy_cap = 0;
    HIP_TRY(c, hipHostMalloc((void **)&s.h_xy, n_xy * sizeof(uint32_t), hipHostMallocDefault));
    HIP_TRY(c, hipMalloc((void **)&s.d_xy, n_xy * sizeof(uint32_t)));
    s.xy_cap = n_xy;
  }
  if (n_bt > s.bt_cap) {
    (void)hipFree(s.d_bt);
    s.d_bt = nullptr;
    s.bt_cap = 0;
    HIP_TRY(c, hipMalloc((void **)&s.d_bt, n_bt * sizeof(long long)));
    s.bt_cap = n_bt;
  }
  if (pinned && n_bt > s.h_bt_cap) {
    if (s.h_bt) HIP_TRY(c, hipHostFree(s.h_bt));
    s.h_bt = nullptr;
    s.h_bt_cap = 0;
    HIP_TRY(c, hipHostMalloc((void **)&s.h_bt, n_bt * sizeof(long long), hipHostMallocDefault));
    s.h_bt_cap = n_bt;
  }
  return CMX_OK;
}

// host arrays (SoA, or the host's own records): validate EVERYTHING first -- a call that fails adds nothing -- then pack slice
// i+1 on the host pool and upload it on the copy stream while the vote kernel of slice i runs
static int recon_add_host(cmx_ctx *c, const EventSource &src, bool grad) {
  ReconState *r = c->recon;
  if (int rc0 = recon_pass_enter(c, r, grad)) return rc0;
  // argument checks + EVERY coordinate handed in inside the sensor, those the sampling or the one-event rule skip included: what
  // cmx_backend_set_window checks when it sub-samples, here at every rate (cmax_hip.h)
  int rc = check_events(c, src);
  if (rc) return rc;
  const int64_t n = src.n;
  BatchPlan p;
  int slice_batches = 1;
  rc = recon_plan(c, r, n, &p, &slice_batches);
  if (rc) return rc;
  if (p.nb == 0) return CMX_OK;
  const int B = r->B;
  const BatchTimeError bad = src.view([&](const auto &v) { return batch_times(v, n, B, 0, p.nb, &r->sup, [](int64_t, long long) {}); });
  if (bad.kind) return fail_batch_time(c, bad, r->sup);
  ReconGatherArgs ga = recon_gather_args(c, r);
  ReconArgs &a = ga.ev;
  // From here on only a runtime error (CMX_ERR_HIP) can end the call, and slices queued before it have voted: "a call that fails
  // adds nothing" is the contract of the validation above.  The slots are left idle either way.
  auto vote_slices = [&]() -> int {
  int k = 0;
  for (int b_lo = 0; b_lo < p.nb; b_lo += slice_batches, k++) {
    const Slice sl = slice_at(p, n, b_lo, slice_batches);
    const int b_hi = sl.b_hi, nbs = b_hi - b_lo;
    const int64_t ev_off = sl.ev_first, np_s = sl.n;
    ReconSlot &s = r->slot[k & 1];
    if (s.busy) { HIP_TRY(c, hipEventSynchronize(s.done)); s.busy = false; }  // its previous slice has been voted
    rc = slot_ensure(c, s, (size_t)np_s, (size_t)nbs, true);
    if (rc) return rc;
    uint32_t *xy = s.h_xy;
    long long *bt = s.h_bt;
    src.view([&](const auto &v) {  // (validated above: neither pass finds anything)
      batch_times(v, n, B, b_lo, b_hi, nullptr, [&](int64_t b, long long tb) { bt[b - b_lo] = tb; });
      return pack_events<false>(v.from(ev_off), n - ev_off, nbs, B, r->rate, (unsigned)c->W, (unsigned)c->H, 0, xy);
    });
    HIP_TRY(c, hipMemcpyAsync(s.d_xy, xy, (size_t)np_s * sizeof(uint32_t), hipMemcpyHostToDevice, r->copy_stream));
    HIP_TRY(c, hipMemcpyAsync(s.d_bt, bt, (size_t)nbs * sizeof(long long), hipMemcpyHostToDevice, r->copy_stream));
    HIP_TRY(c, hipEventRecord(s.up, r->copy_stream));
    HIP_TRY(c, hipStreamWaitEvent(c->stream, s.up, 0));
    a.xy = s.d_xy; a.stride = 0;
    a.batch_t = s.d_bt; a.nb = nbs;
    a.n = (int)np_s;
    rc = queue_slice(c, r, ga, grad);
    if (rc) return rc;
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipEventRecord(s.done, c->stream));
    s.busy = true;
  }
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return CMX_OK;
  };
  rc = vote_slices();
  if (rc) { (void)hipStreamSynchronize(r->copy_stream); (void)hipStreamSynchronize(c->stream); }
  r->slot[0].busy = r->slot[1].busy = false;
  if (rc) return rc;
  (grad ? r->g_sampled : r->n_sampled) += p.n_packed;
  return CMX_OK;
}

// events already on the device (event store): batch times and their validation by launch_be_batch_times, slice by slice into
// one slice-sized table; the error words are read before the first vote kernel of the call is queued
static int recon_add_store(cmx_ctx *c, const EventSource &src, bool grad) {
  ReconState *r = c->recon;
  if (int rc0 = recon_pass_enter(c, r, grad)) return rc0;
  const int64_t n = src.n;
  if (n < 0 || n > kMaxEvents) return fail(c, CMX_ERR_INVALID_ARG, "bad event count %lld", (long long)n);
  BatchPlan p;
  int slice_batches = 1;
  int rc = recon_plan(c, r, n, &p, &slice_batches);
  if (rc) return rc;
  if (p.nb == 0) return CMX_OK;
  const int B = r->B;
  ReconSlot &s = r->slot[0];
  rc = slot_ensure(c, s, 0, (size_t)(p.nb < slice_batches ? p.nb : slice_batches), false);
  if (rc) return rc;
  auto slice_times = [&](int b_lo, const Slice &sl, bool clear_err) {
    return queue_batch_times(c, src.d_t + sl.ev_first, sl.ev_n, B, sl.b_hi - b_lo, r->sup, s.d_bt, r->d_err, clear_err);
  };
  for (int b_lo = 0; b_lo < p.nb && !rc; b_lo += slice_batches) rc = slice_times(b_lo, slice_at(p, n, b_lo, slice_batches), b_lo == 0);
  if (rc) return rc;
  HIP_TRY(c, hipGetLastError());
  BatchTimeError bad;
  rc = read_batch_errors(c, r->d_err, &bad);
  if (rc) return rc;
  if (bad.kind) return fail_batch_time(c, bad, r->sup, /*with_event=*/false);  // (its index would be relative to a slice)
  ReconGatherArgs ga = recon_gather_args(c, r);
  ReconArgs &a = ga.ev;
  const bool one_slice = p.nb <= slice_batches;  // (its batch times are those the validation pass has just written)
  for (int b_lo = 0; b_lo < p.nb; b_lo += slice_batches) {
    const Slice sl = slice_at(p, n, b_lo, slice_batches);
    if (!one_slice) {
      rc = slice_times(b_lo, sl, false);
      if (rc) return rc;
    }
    a.xy = src.d_xy + sl.ev_first; a.stride = r->rate;
    a.batch_t = s.d_bt; a.nb = sl.b_hi - b_lo;
    a.n = (int)sl.n;
    rc = queue_slice(c, r, ga, grad);
    if (rc) return rc;
  }
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  (grad ? r->g_sampled : r->n_sampled) += p.n_packed;
  return CMX_OK;
}

// the six entry points that hand events over: the front door, the call's own way to its source (host arrays, the host's records,
// a range of an event store -- with that form's argument checks), then the vote pass or the gradient pass over it
template <typename MakeSource>
static int recon_add_entry(cmx_ctx *c, bool grad, MakeSource make) {
  int rc = recon_enter(c, true);
  if (rc) return rc;
  EventSource src;
  rc = make(&src);
  if (rc) return rc;
  return src.on_device() ? recon_add_store(c, src, grad) : recon_add_host(c, src, grad);
}
static int recon_add_arrays(cmx_ctx *c, bool grad, int64_t n, const uint16_t *x, const uint16_t *y, const int64_t *t_ns) {
  return recon_add_entry(c, grad, [&](EventSource *src) { *src = EventSource::arrays(n, x, y, t_ns); return (int)CMX_OK; });
}
static int recon_add_records(cmx_ctx *c, bool grad, int64_t n, const void *events, const cmx_aos_layout *layout) {
  return recon_add_entry(c, grad, [&](EventSource *src) { return make_aos(c, n, events, layout, src); });
}
// (the vote kernel reads the store's own packed events -- the per-batch sampling is an index map, nothing is copied -- and
// launch_be_batch_times forms and validates the batch times)
static int recon_add_range(cmx_ctx *c, bool grad, const cmx_events *e, int64_t first, int64_t count) {
  return recon_add_entry(c, grad, [&](EventSource *src) { return store_source(c, e, first, count, src); });
}
int cmx_backend_recon_add(cmx_ctx *c, int64_t n, const uint16_t *x, const uint16_t *y, const int64_t *t_ns) {
  return recon_add_arrays(c, false, n, x, y, t_ns);
}
int cmx_backend_recon_grad_add(cmx_ctx *c, int64_t n, const uint16_t *x, const uint16_t *y, const int64_t *t_ns) {
  return recon_add_arrays(c, true, n, x, y, t_ns);
}
int cmx_backend_recon_add_aos(cmx_ctx *c, int64_t n, const void *events, const cmx_aos_layout *layout) {
  return recon_add_records(c, false, n, events, layout);
}
int cmx_backend_recon_grad_add_aos(cmx_ctx *c, int64_t n, const void *events, const cmx_aos_layout *layout) {
  return recon_add_records(c, true, n, events, layout);
}
int cmx_backend_recon_add_from(cmx_ctx *c, const cmx_events *e, int64_t first, int64_t count) {
  return recon_add_range(c, false, e, first, count);
}
int cmx_backend_recon_grad_add_from(cmx_ctx *c, const cmx_events *e, int64_t first, int64_t count) {
  return recon_add_range(c, true, e, first, count);
}

// ---- per-event export (cmx_backend_recon_warp*): where every event handed in lands under the knots the reconstruction
// holds now.  The batch plan, the batch times, the slices and the validation of add*; ALL events of a slice reach the kernel (the
// host paths pack at rate 1, the store is read in place), the true rate only decides the SAMPLED bit.  Nothing of the reconstruction
// but the knots is read and nothing of it is written: no recon_pass_enter, no counter, no plane.
static int warp_slot_ensure(cmx_ctx *c, ReconState *r, ReconWarpSlot &s, size_t n) {
  if (!r->down_stream) HIP_TRY(c, hipStreamCreateWithFlags(&r->down_stream, hipStreamNonBlocking));
  if (!s.kdone) HIP_TRY(c, hipEventCreateWithFlags(&s.kdone, hipEventDisableTiming));
  if (!s.down) HIP_TRY(c, hipEventCreateWithFlags(&s.down, hipEventDisableTiming));
  if (n <= s.cap) return CMX_OK;
  if (s.h_xy) HIP_TRY(c, hipHostFree(s.h_xy));
  if (s.h_fl) HIP_TRY(c, hipHostFree(s.h_fl));
  (void)hipFree(s.d_xy);
  (void)hipFree(s.d_fl);
  s.h_xy = s.d_xy = nullptr; s.h_fl = s.d_fl = nullptr; s.cap = 0;
  HIP_TRY(c, hipHostMalloc(&s.h_xy, n * 2 * sizeof(double), hipHostMallocDefault));
  HIP_TRY(c, hipHostMalloc((void **)&s.h_fl, n, hipHostMallocDefault));
  HIP_TRY(c, hipMalloc(&s.d_xy, n * 2 * sizeof(double)));
  HIP_TRY(c, hipMalloc((void **)&s.d_fl, n));
  s.cap = n;
  return CMX_OK;
}

static int recon_warp_source(cmx_ctx *c, const EventSource &src, int format, void *xy_out, unsigned char *flags_out, bool dev_out) {
  ReconState *r = c->recon;
  const bool store = src.on_device();
  const int64_t n = src.n;
  int rc = CMX_OK;
  if (store) {
    if (n < 0 || n > kMaxEvents) return fail(c, CMX_ERR_INVALID_ARG, "bad event count %lld", (long long)n);
  } else {
    rc = check_events(c, src);
    if (rc) return rc;
  }
  if (n > 0 && !xy_out) return fail(c, CMX_ERR_INVALID_ARG, "null coordinate output");
  if (n == 0) return CMX_OK;
  BatchPlan p;
  int slice_batches = 1;
  rc = recon_plan(c, r, n, &p, &slice_batches);
  if (rc) return rc;
  const int B = r->B;
  const bool lone = (int64_t)p.nb * B < n;  // the trailing event no batch holds (n = nb B + 1)
  const long long lone_t = lone ? (long long)src.view([&](const auto &v) { return v.T(n - 1); }) : 0;  // (store: its host mirror)
  ReconSlot &s0 = r->slot[0];
  auto slice_times = [&](int b_lo, const Slice &sl, bool clear_err) {
    return queue_batch_times(c, src.d_t + sl.ev_first, sl.ev_n, B, sl.b_hi - b_lo, r->sup, s0.d_bt, r->d_err, clear_err);
  };
  if (store && p.nb > 0) {
    rc = slot_ensure(c, s0, 0, (size_t)(p.nb < slice_batches ? p.nb : slice_batches), false);
    if (rc) return rc;
    for (int b_lo = 0; b_lo < p.nb && !rc; b_lo += slice_batches) rc = slice_times(b_lo, slice_at(p, n, b_lo, slice_batches), b_lo == 0);
    if (rc) return rc;
    HIP_TRY(c, hipGetLastError());
    BatchTimeError bad;
    rc = read_batch_errors(c, r->d_err, &bad);
    if (rc) return rc;
    if (bad.kind) return fail_batch_time(c, bad, r->sup, /*with_event=*/false);
  } else if (p.nb > 0) {
    const BatchTimeError bad = src.view([&](const auto &v) { return batch_times(v, n, B, 0, p.nb, &r->sup, [](int64_t, long long) {}); });
    if (bad.kind) return fail_batch_time(c, bad, r->sup);
  }
  if (lone) {  // its own time is its pose time: inside the spline like a batch time
    const long long st = lone_t - r->sup.start_ns;
    if (st < 0 || st / r->sup.dt_ns + r->sup.order > r->sup.K) return fail_batch_time(c, BatchTimeError{CMX_ERR_SPLINE_RANGE, lone_t}, r->sup);
  }
  // From here on only a runtime error (CMX_ERR_HIP) can end the call.
  const bool f32 = format == CMX_WARP_F32;
  const size_t pair = f32 ? 2 * sizeof(float) : 2 * sizeof(double);
  ReconWarpArgs g{};
  g.ev = recon_args(c, r);
  g.ev.per_batch = B; g.ev.stride = 0;
  g.ev.run = recon_run(B);
  g.rate = r->rate;
  g.lone_t = lone_t;
  g.f32 = f32 ? 1 : 0;
  struct Pending { ReconWarpSlot *o = nullptr; int64_t first = 0, count = 0; } pend;
  auto finish = [&](Pending &q) -> int {  // the download of a slice is complete: into the caller's arrays
    if (!q.o) return CMX_OK;
    HIP_TRY(c, hipEventSynchronize(q.o->down));
    const char *hx = static_cast<const char *>(q.o->h_xy);
    const unsigned char *hf = q.o->h_fl;
    char *ox = static_cast<char *>(xy_out) + (size_t)q.first * pair;
    unsigned char *of = flags_out ? flags_out + q.first : nullptr;
    parallel_ranges(q.count, [=](int64_t a0, int64_t a1) {
      memcpy(ox + (size_t)a0 * pair, hx + (size_t)a0 * pair, (size_t)(a1 - a0) * pair);
      if (of) memcpy(of + a0, hf + a0, (size_t)(a1 - a0));
    });
    q.o = nullptr;
    return CMX_OK;
  };
  auto slices = [&]() -> int {
    const bool one_slice = p.nb <= slice_batches;  // (store: its batch times are those the validation pass has just written)
    int k = 0;
    for (int b_lo = 0; b_lo < p.nb || k == 0; b_lo += slice_batches, k++) {
      Slice sl;
      if (p.nb > 0) sl = slice_at(p, n, b_lo, slice_batches);
      else sl.ev_n = n;  // (n == 1: the lone event alone)
      const int b_hi = sl.b_hi, nbs = b_hi - b_lo;
      const int64_t ev_off = sl.ev_first, ev_n = sl.ev_n;
      const bool with_lone = lone && b_hi == p.nb;
      if (store) {
        if (!one_slice) {
          rc = slice_times(b_lo, sl, false);
          if (rc) return rc;
        }
        g.ev.xy = src.d_xy + ev_off;
        g.ev.batch_t = s0.d_bt;
      } else {
        ReconSlot &s = r->slot[k & 1];
        if (s.busy) { HIP_TRY(c, hipEventSynchronize(s.done)); s.busy = false; }  // its previous slice has been read
        rc = slot_ensure(c, s, (size_t)ev_n, (size_t)nbs, true);
        if (rc) return rc;
        uint32_t *xy = s.h_xy;
        long long *bt = s.h_bt;
        src.view([&](const auto &v) {  // (validated above: neither pass finds anything)
          if (nbs > 0) batch_times(v, n, B, b_lo, b_hi, nullptr, [&](int64_t b, long long tb) { bt[b - b_lo] = tb; });
          const auto vs = v.from(ev_off);
          unsigned outside = pack_events<false>(vs, n - ev_off, nbs, B, 1, (unsigned)c->W, (unsigned)c->H, 0, xy);  // every event: rate 1
          if (with_lone) xy[ev_n - 1] = pack_word<false>(vs, ev_n - 1, (unsigned)c->W, (unsigned)c->H, 0, outside);
          return outside;
        });
        HIP_TRY(c, hipMemcpyAsync(s.d_xy, xy, (size_t)ev_n * sizeof(uint32_t), hipMemcpyHostToDevice, r->copy_stream));
        if (nbs > 0) HIP_TRY(c, hipMemcpyAsync(s.d_bt, bt, (size_t)nbs * sizeof(long long), hipMemcpyHostToDevice, r->copy_stream));
        HIP_TRY(c, hipEventRecord(s.up, r->copy_stream));
        HIP_TRY(c, hipStreamWaitEvent(c->stream, s.up, 0));
        g.ev.xy = s.d_xy;
        g.ev.batch_t = s.d_bt;
      }
      g.ev.nb = nbs;
      g.ev.n = (int)ev_n;
      g.lone = with_lone ? 1 : 0;
      ReconWarpSlot *o = nullptr;
      if (dev_out) {
        g.xy_out = static_cast<char *>(xy_out) + (size_t)ev_off * pair;
        g.flags_out = flags_out ? flags_out + ev_off : nullptr;
      } else {
        o = &r->wslot[k & 1];  // (free: the slice before the last was finished while the last one ran)
        rc = warp_slot_ensure(c, r, *o, (size_t)ev_n);
        if (rc) return rc;
        g.xy_out = o->d_xy;
        g.flags_out = flags_out ? o->d_fl : nullptr;
      }
      g.vec = (uintptr_t)g.xy_out % (f32 ? 8 : 16) == 0 ? 1 : 0;
      launch_recon_warp(g, c->stream);
      HIP_TRY(c, hipGetLastError());
      if (!store) {
        ReconSlot &s = r->slot[k & 1];
        HIP_TRY(c, hipEventRecord(s.done, c->stream));
        s.busy = true;
      }
      if (o) {
        HIP_TRY(c, hipEventRecord(o->kdone, c->stream));
        HIP_TRY(c, hipStreamWaitEvent(r->down_stream, o->kdone, 0));
        HIP_TRY(c, hipMemcpyAsync(o->h_xy, o->d_xy, (size_t)ev_n * pair, hipMemcpyDeviceToHost, r->down_stream));
        if (flags_out) HIP_TRY(c, hipMemcpyAsync(o->h_fl, o->d_fl, (size_t)ev_n, hipMemcpyDeviceToHost, r->down_stream));
        HIP_TRY(c, hipEventRecord(o->down, r->down_stream));
        rc = finish(pend);  // the slice before this one, while this one runs
        if (rc) return rc;
        pend.o = o; pend.first = ev_off; pend.count = ev_n;
      }
    }
    rc = finish(pend);
    if (rc) return rc;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return CMX_OK;
  };
  rc = slices();
  if (rc) {
    (void)hipStreamSynchronize(r->copy_stream);
    (void)hipStreamSynchronize(c->stream);
    if (r->down_stream) (void)hipStreamSynchronize(r->down_stream);
  }
  r->slot[0].busy = r->slot[1].busy = false;
  return rc;
}

template <typename MakeSource>
static int recon_warp_entry(cmx_ctx *c, int format, void *xy_out, unsigned char *flags_out, bool dev_out, MakeSource make) {
  int rc = recon_enter(c, true);
  if (rc) return rc;
  if (format != CMX_WARP_F64 && format != CMX_WARP_F32) return fail(c, CMX_ERR_INVALID_ARG, "unknown output format %d", format);
  EventSource src;
  rc = make(&src);
  if (rc) return rc;
  return recon_warp_source(c, src, format, xy_out, flags_out, dev_out);
}
int cmx_backend_recon_warp(cmx_ctx *c, int64_t n, const uint16_t *x, const uint16_t *y, const int64_t *t_ns, int format, void *xy_out,
                           unsigned char *flags_out) {
  return recon_warp_entry(c, format, xy_out, flags_out, false,
                          [&](EventSource *src) { *src = EventSource::arrays(n, x, y, t_ns); return (int)CMX_OK; });
}
int cmx_backend_recon_warp_aos(cmx_ctx *c, int64_t n, const void *events, const cmx_aos_layout *layout, int format, void *xy_out,
                               unsigned char *flags_out) {
  return recon_warp_entry(c, format, xy_out, flags_out, false, [&](EventSource *src) { return make_aos(c, n, events, layout, src); });
}
int cmx_backend_recon_warp_from(cmx_ctx *c, const cmx_events *e, int64_t first, int64_t count, int format, void *xy_out,
                                unsigned char *flags_out) {
  return recon_warp_entry(c, format, xy_out, flags_out, false, [&](EventSource *src) { return store_source(c, e, first, count, src); });
}
int cmx_backend_recon_warp_from_device(cmx_ctx *c, const cmx_events *e, int64_t first, int64_t count, int format, void *d_xy_out,
                                       unsigned char *d_flags_out) {
  return recon_warp_entry(c, format, d_xy_out, d_flags_out, true, [&](EventSource *src) { return store_source(c, e, first, count, src); });
}

// events of the binding have been released (cmx_backend_recon_release_head): their votes live in the frozen base alone, so whatever
// would drop or rebuild that base -- and keep the binding -- is refused
static int recon_refuse_released(cmx_ctx *c, const ReconState *r, const char *what) {
  if (!r->bound || r->bnd.rel_batches == 0) return CMX_OK;
  return fail(c, CMX_ERR_STATE, "%s would lose the %lld events released from the binding (cmx_backend_recon_release_head)", what,
              (long long)r->bnd.rel_events);
}

int cmx_backend_recon_restart(cmx_ctx *c, const double *knots_xyzw) {
  int rc = recon_enter(c, true);
  if (rc) return rc;
  if (!knots_xyzw) return fail(c, CMX_ERR_INVALID_ARG, "null knot array");
  rc = recon_refuse_released(c, c->recon, "restart");
  if (rc) return rc;
  frozen_drop(c, c->recon);  // (new knots: what the frozen batches voted no longer holds)
  return recon_start_over(c, c->recon, knots_xyzw);
}

// restart that may lengthen the spline and keeps a frozen head: everything sized by K grows with it -- the knots and
// their logarithms, the 2 x 3K sums, the solve's staging (allocated again by the next solve) -- before anything changes
int cmx_backend_recon_extend(cmx_ctx *c, int K_new, const double *knots_xyzw) {
  int rc = recon_enter(c, true);
  if (rc) return rc;
  ReconState *r = c->recon;
  const int K = r->sup.K;
  if (!knots_xyzw) return fail(c, CMX_ERR_INVALID_ARG, "null knot array");
  if (K_new < K || K_new > (1 << 28)) return fail(c, CMX_ERR_INVALID_ARG, "K_new=%d outside [%d, 2^28]", K_new, K);
  const ReconFrozen &fz = r->frozen;
  if (fz.num_fixed > 0 && memcmp(knots_xyzw, fz.knots.data(), (size_t)fz.num_fixed * sizeof(Quat)) != 0)
    return fail(c, CMX_ERR_INVALID_ARG, "the first %d knots differ from those the head was frozen at", fz.num_fixed);
  if (K_new > K) {
    Quat *knots = nullptr;
    double *delta = nullptr, *gsum = nullptr;
    hipError_t e = hipMalloc((void **)&knots, (size_t)K_new * sizeof(Quat));
    if (e == hipSuccess) e = hipMalloc((void **)&delta, (size_t)(K_new - 1) * 3 * sizeof(double));
    if (e == hipSuccess && r->d_gsum) e = hipMalloc((void **)&gsum, 2 * 3 * (size_t)K_new * sizeof(double));
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);  // (nothing queued reads the old ones any more)
    if (e != hipSuccess) {
      (void)hipFree(knots); (void)hipFree(delta); (void)hipFree(gsum);
      return fail(c, CMX_ERR_HIP, "growing the spline to %d knots: %s", K_new, hipGetErrorString(e));
    }
    (void)hipFree(r->d_knots); (void)hipFree(r->d_delta); (void)hipFree(r->d_gsum);
    r->d_knots = knots; r->d_delta = delta; r->d_gsum = gsum;
    r->solve.release();
    r->sup.K = K_new;
  }
  if (fz.num_fixed == 0) frozen_drop(c, r);  // (as restart: a base allocated without a head goes)
  return recon_start_over(c, r, knots_xyzw);
}

static void recon_refresh_plane(cmx_ctx *c, ReconState *r);

// taps and G^T 1 factors of the reconstruction for this sigma (setup_blur's, in buffers of its own)
static int recon_setup_blur(cmx_ctx *c, ReconState *r, double sigma) {
  if (r->sigma_built == sigma && sigma >= 0) return CMX_OK;
  int radius = 0;
  float taps[2 * kMaxRadius + 1] = {1.f};
  if (sigma > 0) {
    const int rc = blur_taps(c, sigma, taps, &radius);
    if (rc) return rc;
  }
  r->sigma_built = -1.0;
  r->grad_open = false;  // (an open gradient pass was made for the other sigma's Jt and border factors)
  r->radius = radius;
  memcpy(r->taps, taps, sizeof(taps));
  if (!r->d_cx) HIP_TRY(c, hipMalloc((void **)&r->d_cx, (size_t)c->Wp * sizeof(float)));
  if (!r->d_cy) HIP_TRY(c, hipMalloc((void **)&r->d_cy, (size_t)c->Hp * sizeof(float)));
  std::vector<float> vx((size_t)c->Wp), vy((size_t)c->Hp);
  gt1_factors(taps, radius, c->Wp, vx.data());
  gt1_factors(taps, radius, c->Hp, vy.data());
  HIP_TRY(c, hipStreamSynchronize(c->stream));  // (nothing queued reads the factors any more)
  HIP_TRY(c, hipMemcpy(r->d_cx, vx.data(), vx.size() * sizeof(float), hipMemcpyHostToDevice));
  HIP_TRY(c, hipMemcpy(r->d_cy, vy.data(), vy.size() * sizeof(float), hipMemcpyHostToDevice));
  r->sigma_built = sigma;
  return CMX_OK;
}
// ... and what a gradient at this sigma needs on top of it: G^T folds single reflections, so the panorama is larger than the kernel
static int recon_grad_precheck(cmx_ctx *c, ReconState *r, double sigma) {
  const int rc = recon_setup_blur(c, r, sigma);
  if (rc) return rc;
  if (!(c->Wp > 2 * r->radius + 1 && c->Hp > 2 * r->radius + 1))
    return fail(c, CMX_ERR_INVALID_ARG, "panorama %d x %d too small for the adjoint gradient at blur radius %d", c->Wp, c->Hp, r->radius);
  return CMX_OK;
}

// The image pass over the plane as accumulated so far: contrast of GaussianBlur(plane, sigma), and with want_grad
// Jt = G^T (G plane) for the gradient pass it opens.  The plane is read only.
// Everything of it up to the wait: queued on the stream, contrast and mean on their way into cm[2] (host memory that stays valid
// until the caller has waited for the stream); with want_grad the gradient pass is open from here on, and r->mu is the caller's to
// set from cm[1] after its wait.
static int recon_contrast_queue(cmx_ctx *c, ReconState *r, double blur_sigma, int contrast_measure, int want_grad, double *cm) {
  if (!std::isfinite(blur_sigma)) return fail(c, CMX_ERR_INVALID_ARG, "blur_sigma is not finite");
  int rc = want_grad ? recon_grad_precheck(c, r, blur_sigma) : recon_setup_blur(c, r, blur_sigma);
  if (rc) return rc;
  const int W = c->Wp, H = c->Hp, rad = r->radius;
  const size_t np = (size_t)W * H;
  ImgAdjArgs ia{};
  ImgArgs &a = ia.img;
  a.W = W; a.H = H; a.r = rad;
  memcpy(a.taps, r->taps, sizeof(a.taps));
  a.src_a = r->d_plane;
  a.P = 0;
  a.tiles_x = (W + kTileX - 1) / kTileX;
  a.tiles_y = (H + kTileY - 1) / kTileY;
  a.nblk = a.tiles_x * a.tiles_y;
  if (!r->d_tflags) HIP_TRY(c, hipMalloc((void **)&r->d_tflags, (size_t)a.nblk));
  if (!r->d_partials) HIP_TRY(c, hipMalloc((void **)&r->d_partials, 2 * (size_t)a.nblk * sizeof(double)));
  if (!r->d_cm) HIP_TRY(c, hipMalloc((void **)&r->d_cm, 2 * sizeof(double)));
  if (a.nblk > kTileListMin && !r->d_tile_list) {
    HIP_TRY(c, hipMalloc((void **)&r->d_tile_list, (2 * (size_t)a.nblk + 8) * sizeof(unsigned)));  // list + dense scratch (launch_tile_list)
    HIP_TRY(c, hipMalloc((void **)&r->d_tile_count, 2 * sizeof(unsigned)));
  }
  if (want_grad) {
    if (!r->d_jt) {  // tiles the image pass skips keep whatever they held: finite from the start
      HIP_TRY(c, hipMalloc((void **)&r->d_jt, np * sizeof(float)));
      HIP_TRY(c, hipMemsetAsync(r->d_jt, 0, np * sizeof(float), c->stream));
    }
    if (!r->d_gsum) HIP_TRY(c, hipMalloc((void **)&r->d_gsum, 2 * 3 * (size_t)r->sup.K * sizeof(double)));
    if (!r->d_voted) HIP_TRY(c, hipMalloc((void **)&r->d_voted, sizeof(unsigned long long)));
  }
  recon_refresh_plane(c, r);
  HIP_TRY(c, hipMemsetAsync(r->d_tflags, 0, (size_t)a.nblk, c->stream));
  launch_tile_flags(r->d_plane, W, H, r->d_tflags, c->stream);
  a.flags_cur = r->d_tflags;
  a.partials = r->d_partials;
  if (r->d_tile_list) {  // tile order: the order the moment rows are summed in does not depend on the run
    launch_tile_list(a, want_grad ? 2 * rad : rad, r->d_tile_list, r->d_tile_count, r->d_tile_count + 1, /*ordered=*/true, c->stream);
    a.tile_list = r->d_tile_list;
    a.tile_count = r->d_tile_count;
  }
  if (want_grad) {
    ia.jt = r->d_jt;
    launch_image_adjoint(ia, c->stream);
  } else {
    launch_image_moments(a, c->stream);
  }
  launch_recon_moments_finalize(r->d_partials, a.nblk, a.tile_count, (double)np, contrast_measure, r->d_cm, c->stream);
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipMemcpyAsync(cm, r->d_cm, 2 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  if (want_grad) {
    HIP_TRY(c, hipMemsetAsync(r->d_gsum, 0, 2 * 3 * (size_t)r->sup.K * sizeof(double), c->stream));
    HIP_TRY(c, hipMemsetAsync(r->d_voted, 0, sizeof(unsigned long long), c->stream));
    r->measure = contrast_measure;
    r->g_sampled = 0;
    r->g_num_fixed = 0;
    r->grad_open = true;
  }
  return CMX_OK;
}
int cmx_backend_recon_contrast(cmx_ctx *c, double blur_sigma, int contrast_measure, int want_grad, double *contrast) {
  int rc = recon_enter(c, true);
  if (rc) return rc;
  if (!contrast) return fail(c, CMX_ERR_INVALID_ARG, "null output");
  ReconState *r = c->recon;
  double cm[2] = {0, 0};
  rc = recon_contrast_queue(c, r, blur_sigma, contrast_measure, want_grad, cm);
  if (rc) return rc;
  HIP_TRY(c, recon_wait(c, r));
  *contrast = cm[0];
  if (want_grad) r->mu = cm[1];
  return CMX_OK;
}

// grad = (2/N)(S1 - mu S2) once the gradient pass has seen exactly the plane's events
int cmx_backend_recon_grad_get(cmx_ctx *c, double *grad) {
  int rc = recon_enter(c, true);
  if (rc) return rc;
  if (!grad) return fail(c, CMX_ERR_INVALID_ARG, "null output");
  ReconState *r = c->recon;
  if (!r->grad_open) return fail(c, CMX_ERR_STATE, "no gradient pass is open");
  unsigned long long cnt[2] = {0, 0};
  HIP_TRY(c, hipMemcpyAsync(&cnt[0], r->d_inside, sizeof(cnt[0]), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipMemcpyAsync(&cnt[1], r->d_voted, sizeof(cnt[1]), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, recon_wait(c, r));
  // (a frozen evaluation's pass starts both of its counts from the frozen head's -- bound_eval -- so the test below reads
  //  "base plus active against the plane" there)
  if (r->g_sampled != r->n_sampled || cnt[0] != cnt[1])
    return fail(c, CMX_ERR_STATE, "the gradient pass saw %lld sampled / %llu voting events, the plane holds %lld / %llu: feed it the same events in the same cuts",
                (long long)r->g_sampled, cnt[1], (long long)r->n_sampled, cnt[0]);
  const size_t P = 3 * (size_t)r->sup.K;
  std::vector<double> s(2 * P);
  r->host_waits++;
  HIP_TRY(c, hipMemcpy(s.data(), r->d_gsum, 2 * P * sizeof(double), hipMemcpyDeviceToHost));
  const double N = (double)c->Wp * (double)c->Hp, mu = r->measure == CMX_MEAN_SQUARE ? 0.0 : r->mu;
  for (size_t k = 0; k < P; k++) grad[k] = 2.0 * (s[k] - (mu != 0.0 ? mu * s[P + k] : 0.0)) / N;
  for (size_t k = 0; k < 3 * (size_t)r->g_num_fixed; k++) grad[k] = 0.0;  // (active batches next to the cut do reach fixed knots)
  return CMX_OK;
}

// restart (when knots are given) + add_from + contrast + (grad_add_from + grad_get): the form an optimiser calls per trial point
int cmx_backend_recon_eval_from(cmx_ctx *c, const cmx_events *e, int64_t first, int64_t count, const double *knots_xyzw, double blur_sigma,
                                int contrast_measure, double *contrast, double *grad) {
  int rc = recon_enter(c, true);
  if (rc) return rc;
  if (!contrast) return fail(c, CMX_ERR_INVALID_ARG, "null output");
  ReconState *r = c->recon;
  if (knots_xyzw) {
    rc = recon_refuse_released(c, r, "eval_from with knots");
    if (rc) return rc;
  }
  if (grad) {  // (before anything is changed: the one argument error the later steps would find)
    rc = recon_grad_precheck(c, r, blur_sigma);
    if (rc) return rc;
  }
  EventSource src;
  rc = store_source(c, e, first, count, &src);
  if (rc) return rc;
  if (knots_xyzw) rc = cmx_backend_recon_restart(c, knots_xyzw);
  if (!rc) rc = recon_add_store(c, src, false);
  if (!rc) rc = cmx_backend_recon_contrast(c, blur_sigma, contrast_measure, grad != nullptr, contrast);
  if (!rc && grad) rc = recon_add_store(c, src, true);
  if (!rc && grad) rc = cmx_backend_recon_grad_get(c, grad);
  return rc;
}

// ---- bound events: hand the events over ONCE, evaluate them many times (an optimiser's trial points) with the votes made through LDS
// bind_from   validation of recon_add_from, then the sampled events of the range, packed in time order, and their batch times into
//             memory of the reconstruction's own, with a TileSort reserved for them; everything is built beside an earlier binding,
//             which is replaced only once nothing can fail any more
// eval_bound  restart + eval_from over the bound events: batch-pose table behind recon_delta, tile sort at the first evaluation and
//             again after one whose votes left their windows (kRebinFallbackFrac), recon_votes_lds, the image pass, and the gather
//             pass over the time-ordered copy in the slices of every add (slice_at)
constexpr int64_t kMaxBoundSampled = 1LL << 30;  // (sorted positions, chunk bounds and keys are 32-bit)

// the open tail of a binding for its next append: the last n raw events, as a store replica or the append's scratch holds them, into
// buffers of the binding's own (queued; large enough, or new ones -- the caller has made sure nothing queued reads the old ones)
static int tail_keep(cmx_ctx *c, ReconBound *b, const uint32_t *d_xy, const int64_t *d_t, int64_t n) {
  if ((size_t)n > b->tail_cap) {
    (void)hipFree(b->d_tail_xy); (void)hipFree(b->d_tail_t);
    b->d_tail_xy = nullptr; b->d_tail_t = nullptr; b->tail_cap = 0;
    HIP_TRY(c, hipMalloc((void **)&b->d_tail_xy, (size_t)n * sizeof(uint32_t)));
    HIP_TRY(c, hipMalloc((void **)&b->d_tail_t, (size_t)n * sizeof(int64_t)));
    b->tail_cap = (size_t)n;
  }
  if (n > 0) {
    HIP_TRY(c, hipMemcpyAsync(b->d_tail_xy, d_xy, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(b->d_tail_t, d_t, (size_t)n * sizeof(int64_t), hipMemcpyDeviceToDevice, c->stream));
  }
  b->tail_n = n;
  return CMX_OK;
}

static int bound_build(cmx_ctx *c, ReconState *r, const EventSource &src, const BatchPlan &p, ReconBound *b) {
  b->n_events = src.n;
  b->plan = p;
  HIP_TRY(c, hipHostMalloc((void **)&b->h_stat, 2 * sizeof(unsigned long long), hipHostMallocDefault));
  b->h_stat[0] = b->h_stat[1] = 0ull;
  const int64_t tail_from = open_tail_from(src.n, p);
  if (src.n > 0) b->t_last = (long long)src.soa.t[src.n - 1];
  if (p.nb == 0) {  // (0 or 1 events: nothing to vote)
    const int rc0 = tail_keep(c, b, src.d_xy, src.d_t, src.n);
    if (rc0) return rc0;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return CMX_OK;
  }
  HIP_TRY(c, hipMalloc((void **)&b->d_bt, (size_t)p.nb * sizeof(long long)));
  b->bt_cap = (size_t)p.nb;
  int rc = queue_batch_times(c, src.d_t, src.n, r->B, p.nb, r->sup, b->d_bt, r->d_err, true);
  if (rc) return rc;
  HIP_TRY(c, hipGetLastError());
  BatchTimeError bad;
  rc = read_batch_errors(c, r->d_err, &bad);
  if (rc) return rc;
  if (bad.kind) return fail_batch_time(c, bad, r->sup, /*with_event=*/false);
  // ---- valid: the copy, the pose table, and the sort's buffers with the chunk table at the back end's chunk size
  const size_t n = (size_t)p.n_packed;
  const int tiles = ((c->Wp + kBinTile - 1) / kBinTile) * ((c->Hp + kBinTile - 1) / kBinTile);
  const int ntiles = 2 * tiles;  // (the back end's sort keys carry the old / new bit: no bound event sets it, half of the bins stay empty)
  HIP_TRY(c, hipMalloc((void **)&b->d_xy, n * sizeof(uint32_t)));
  b->xy_cap = n;
  HIP_TRY(c, hipMalloc((void **)&b->d_poseR, (size_t)p.nb * sizeof(PoseR)));
  rc = tail_keep(c, b, src.d_xy + tail_from, src.d_t + tail_from, src.n - tail_from);
  if (rc) return rc;
  const ChunkPlan cp = plan_chunks(p.n_packed, ntiles, kBackEndChunkDiv);
  b->chunk_events = cp.chunk_events;
  b->max_chunks = (int)cp.max_chunks;  // (n <= 2^30, at most 2^20 tiles: below 2^23)
  rc = b->ts.reserve(c, p.n_packed, ntiles, cp.max_chunks);
  if (rc) return rc;
  // (t_next = the smallest time: no event carries the old flag)
  launch_be_pack_from_store(src.d_xy, reinterpret_cast<const long long *>(src.d_t), (long long)src.n, r->B, r->rate, p.per_batch, (int)n,
                            std::numeric_limits<long long>::min(), b->d_xy, c->stream);
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipStreamSynchronize(c->stream));  // the store may be pushed to, compacted or closed from here on
  return CMX_OK;
}

int cmx_backend_recon_bind_from(cmx_ctx *c, const cmx_events *e, int64_t first, int64_t count) {
  int rc = recon_enter(c, true);
  if (rc) return rc;
  EventSource src;
  rc = store_source(c, e, first, count, &src);
  if (rc) return rc;
  ReconState *r = c->recon;
  (void)recon_pass_enter(c, r, false);  // as every add: an open gradient pass is closed
  if (src.n < 0 || src.n > kMaxEvents) return fail(c, CMX_ERR_INVALID_ARG, "bad event count %lld", (long long)src.n);
  BatchPlan p;
  int slice_batches = 1;
  rc = recon_plan(c, r, src.n, &p, &slice_batches);
  if (rc) return rc;
  if (p.n_packed > kMaxBoundSampled)
    return fail(c, CMX_ERR_INVALID_ARG, "%lld sampled events above the limit of a binding (2^30)", (long long)p.n_packed);
  ReconBound b;
  rc = bound_build(c, r, src, p, &b);
  if (rc) {  // (an earlier binding is intact: nothing of it was touched)
    (void)hipStreamSynchronize(c->stream);
    b.release();
    return rc;
  }
  frozen_drop(c, r);  // (a frozen head is a property of the binding it was cut from)
  r->bnd.release();
  r->bnd = b;
  r->bound = true;
  return CMX_OK;
}

int cmx_backend_recon_unbind(cmx_ctx *c) {
  int rc = recon_enter(c, true);
  if (rc) return rc;
  ReconState *r = c->recon;
  if (!r->bound) return CMX_OK;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  frozen_drop(c, r);
  r->bnd.release();
  r->bound = false;
  return CMX_OK;
}

int cmx_backend_recon_bound_info(cmx_ctx *c, int64_t *n_events, int64_t *n_sampled, int64_t *sorts, double *fallback_frac) {
  int rc = recon_enter(c, true);
  if (rc) return rc;
  const ReconState *r = c->recon;  // (without a binding: all zero)
  if (n_events) *n_events = r->bound ? r->bnd.n_events : 0;
  if (n_sampled) *n_sampled = r->bound ? r->bnd.plan.n_packed : 0;
  if (sorts) *sorts = r->bound ? r->bnd.sorts : 0;
  if (fallback_frac) *fallback_frac = r->bound ? r->bnd.fallback_frac : 0.0;
  return CMX_OK;
}

// the bound events by the destination tile of their vote under the pose table as it stands, and the chunk table
// (be.xy / be.n / be.poseR: all bound events, or with a frozen head the active ones and the pose table from their first batch on --
//  the sort numbers batches from the first event it is given)
static int bound_sort(cmx_ctx *c, ReconBound &b, const BeSplatArgs &be, int chunk_events) {
  TileSortJob job;
  job.be = &be;
  job.tiles_x = (c->Wp + kBinTile - 1) / kBinTile;
  job.tiles = job.tiles_x * ((c->Hp + kBinTile - 1) / kBinTile);
  job.planes_per_tile = 2;
  job.xy = be.xy; job.per_batch = b.plan.per_batch; job.n = be.n;
  job.chunk_events = chunk_events;
  const int rc = b.ts.run(c, job);
  if (rc) return rc;
  b.sorted = true;
  b.sorts++;
  return CMX_OK;
}

// the gradient pass over the bound time-ordered copy: the slices, runs and launches of recon_add_store, with stride 0
// From batch b_first on (0, or a frozen head's first active batch: the slices then start there, so with b_first = 0 they are
// the unbound pass's).  wait = false: queued only, the caller waits.
static int bound_gather(cmx_ctx *c, ReconState *r, int b_first, bool wait) {
  if (int rc0 = recon_pass_enter(c, r, true)) return rc0;
  const ReconBound &b = r->bnd;
  const BatchPlan &p = b.plan;
  const int slice_batches = recon_slice_batches(r);
  ReconGatherArgs ga = recon_gather_args(c, r);
  ReconArgs &a = ga.ev;
  for (int b_lo = b_first; b_lo < p.nb; b_lo += slice_batches) {
    const Slice sl = slice_at(p, b.n_events, b_lo, slice_batches);
    a.xy = b.xy_at(sl.first); a.stride = 0;  // (resident addresses: b_first is never in front of what release_head gave back)
    a.batch_t = b.bt_at(b_lo); a.nb = sl.b_hi - b_lo;
    a.n = (int)sl.n;
    Span sp(c, CMX_T_GATHER);
    const int rc = queue_slice(c, r, ga, true);
    if (rc) return rc;
  }
  HIP_TRY(c, hipGetLastError());
  if (wait) HIP_TRY(c, recon_wait(c, r));
  r->g_sampled += p.packed(b_first, p.nb);
  return CMX_OK;
}

// One evaluation of the binding: cmx_backend_recon_eval_bound's body, and -- with sv set -- a trial point of
// cmx_backend_recon_solve: the same launches in the same order, but the knots come from pinned staging, nothing waits in between,
// the free gradient entries are formed on the device (recon_grad_finalize) and ONE wait at the end delivers contrast, mean, both
// counters and that slice.  With a frozen head the plane starts from the base and every pass walks the active batches alone.
static int bound_eval(cmx_ctx *c, ReconState *r, const double *knots_xyzw, double blur_sigma, int contrast_measure, double *contrast,
                      double *grad, ReconSolve *sv) {
  ReconBound &b = r->bnd;
  const ReconFrozen &fz = r->frozen;
  const bool frozen = fz.num_fixed > 0;
  if (frozen && knots_xyzw && memcmp(knots_xyzw, fz.knots.data(), (size_t)fz.num_fixed * sizeof(Quat)) != 0)
    return fail(c, CMX_ERR_INVALID_ARG, "the first %d knots differ from those the head was frozen at (cmx_backend_recon_freeze_head)",
                fz.num_fixed);
  int rc = recon_start_over(c, r, knots_xyzw, /*from_base=*/true, /*staged=*/sv != nullptr);
  if (rc) return rc;
  const int b0 = frozen ? fz.b_act : 0;
  // `first`: the first active event's packed index since the bind -- where it lies in the resident arrays is xy_at's business
  const int64_t first = frozen ? fz.sampled : 0, n_act = b.plan.n_packed - first;
  if (n_act > 0) {
    ReconArgs a = recon_args(c, r);
    a.batch_t = b.bt_at(b0); a.nb = b.plan.nb - b0;
    {
      Span sp(c, CMX_T_POSE, /*exact=*/true);
      launch_recon_pose_table(a, b.pose_at(b0), c->stream, sp.t0(), sp.t1());
    }
    ReconLdsArgs g{};
    g.cam = a.cam;
    g.cam.poseR = b.pose_at(b0);
    g.cam.xy = b.xy_at(first);
    g.cam.per_batch = b.plan.per_batch;
    g.cam.n = (int)n_act;
    g.cam.order = r->sup.order;
    if (!b.sorted || b.fallback_frac > kRebinFallbackFrac) {
      Span sp(c, CMX_T_BATCH);
      rc = bound_sort(c, b, g.cam, frozen ? fz.chunk_events : b.chunk_events);
      if (rc) return rc;
    }
    g.ev.sxy = b.ts.d_sxy; g.ev.sbatch = b.ts.d_sbatch;
    g.ev.chunks = b.ts.d_chunks; g.ev.nchunks = frozen ? fz.max_chunks : b.max_chunks; g.ev.nchunks_dev = b.ts.d_nchunks;
    g.ev.fallback = b.ts.d_fallback;
    g.ev.fixed = r->deterministic ? r->d_fixed : nullptr;
    g.plane = r->d_plane;
    g.n_inside = r->d_inside;
    HIP_TRY(c, hipMemsetAsync(b.ts.d_fallback, 0, sizeof(unsigned), c->stream));
    {
      Span sp(c, CMX_T_SPLAT, /*exact=*/true);
      launch_recon_votes_lds(g, c->stream, sp.t0(), sp.t1());
    }
    HIP_TRY(c, hipGetLastError());
    // (into pinned memory of the binding's own; complete once the image pass below has waited for the stream)
    b.h_stat[1] = 0ull;
    HIP_TRY(c, hipMemcpyAsync(&b.h_stat[0], r->d_inside, sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(&b.h_stat[1], b.ts.d_fallback, sizeof(unsigned), hipMemcpyDeviceToHost, c->stream));
    r->n_sampled += n_act;
  }
  // the share of the ACTIVE events' votes that left their windows: the frozen head's votes are in the counter, not in the sort
  auto note_fallback = [&]() {
    if (n_act <= 0) { if (frozen) b.fallback_frac = 0.0; return; }
    const unsigned long long act = b.h_stat[0] - (frozen ? fz.inside : 0ull);
    b.fallback_frac = act ? (double)(unsigned)b.h_stat[1] / (double)act : 0.0;
  };
  // a frozen evaluation's gradient pass: both of its counts start from the frozen head's, so that grad_get's test -- sampled and
  // voted counts against the plane's -- holds for base plus active, and the fixed entries are zero by definition
  auto open_frozen_pass = [&]() -> int {
    if (!frozen) return CMX_OK;
    r->g_sampled = fz.sampled;
    r->g_num_fixed = fz.num_fixed;
    HIP_TRY(c, hipMemcpyAsync(r->d_voted, fz.d_inside, sizeof(unsigned long long), hipMemcpyDeviceToDevice, c->stream));
    return CMX_OK;
  };
  if (!sv) {
    rc = cmx_backend_recon_contrast(c, blur_sigma, contrast_measure, grad != nullptr, contrast);
    if (rc && hipStreamSynchronize(c->stream) != hipSuccess) return rc;  // (the two words below are not known to have arrived)
    note_fallback();
    if (!rc && grad) rc = open_frozen_pass();
    if (!rc && grad) rc = bound_gather(c, r, b0, /*wait=*/true);
    if (!rc && grad) rc = cmx_backend_recon_grad_get(c, grad);
    return rc;
  }
  rc = recon_contrast_queue(c, r, blur_sigma, contrast_measure, grad != nullptr, sv->h_cm);
  const size_t P = 3 * (size_t)r->sup.K, p0 = 3 * (size_t)sv->num_fixed;
  if (!rc && grad) rc = open_frozen_pass();
  if (!rc && grad) rc = bound_gather(c, r, b0, /*wait=*/false);
  if (!rc && grad) {
    launch_recon_grad_finalize(r->d_gsum, r->d_cm, (long long)P, (long long)p0, (double)c->Wp * (double)c->Hp,
                               contrast_measure == CMX_MEAN_SQUARE, sv->d_grad, c->stream);
    rc = hipGetLastError() == hipSuccess ? CMX_OK : fail(c, CMX_ERR_HIP, "the gradient finalize could not be queued");
    if (!rc) {
      HIP_TRY(c, hipMemcpyAsync(&sv->h_cnt[0], r->d_inside, sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
      HIP_TRY(c, hipMemcpyAsync(&sv->h_cnt[1], r->d_voted, sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    }
  }
  const hipError_t waited = recon_wait(c, r);  // the evaluation's one wait (a queueing error above: so that nothing is left in flight)
  if (!rc && waited != hipSuccess) rc = fail(c, CMX_ERR_HIP, "the evaluation failed: %s", hipGetErrorString(waited));
  if (rc) return rc;
  note_fallback();
  *contrast = sv->h_cm[0];
  if (grad) {
    r->mu = sv->h_cm[1];
    if (r->g_sampled != r->n_sampled || sv->h_cnt[0] != sv->h_cnt[1])  // (grad_get's test)
      return fail(c, CMX_ERR_STATE, "the gradient pass saw %lld sampled / %llu voting events, the plane holds %lld / %llu",
                  (long long)r->g_sampled, sv->h_cnt[1], (long long)r->n_sampled, sv->h_cnt[0]);
    memcpy(grad, sv->h_grad, (P - p0) * sizeof(double));
  }
  return CMX_OK;
}

int cmx_backend_recon_eval_bound(cmx_ctx *c, const double *knots_xyzw, double blur_sigma, int contrast_measure, double *contrast,
                                 double *grad) {
  int rc = recon_enter(c, true);
  if (rc) return rc;
  ReconState *r = c->recon;
  if (!r->bound) return fail(c, CMX_ERR_STATE, "no events are bound (cmx_backend_recon_bind_from)");
  if (!contrast) return fail(c, CMX_ERR_INVALID_ARG, "null output");
  if (grad) {  // (before anything is changed, as in eval_from)
    rc = recon_grad_precheck(c, r, blur_sigma);
    if (rc) return rc;
  }
  return bound_eval(c, r, knots_xyzw, blur_sigma, contrast_measure, contrast, grad, nullptr);
}

// ---- frozen head
// eval_bound's own vote pass over the batches [b_lo, b_hi) of the binding, at the knots the reconstruction holds, into a base plane
// and its counter ON TOP of what they hold: pose table, the binding's TileSort filled with THOSE events (the next evaluation sorts
// the active ones into it, as it would anyway), LDS votes.  freeze_head: [0, b_act) into a cleared base; advance_head: the batches
// the moved line newly names.  Queued; the caller waits.
static int frozen_vote(cmx_ctx *c, ReconState *r, void *d_base, unsigned long long *d_inside, int b_lo, int b_hi) {
  ReconBound &b = r->bnd;
  const BatchPlan &p = b.plan;
  const int64_t first = p.packed(0, b_lo), n = p.packed(b_lo, b_hi);
  if (n > 0) {
    const int tiles = ((c->Wp + kBinTile - 1) / kBinTile) * ((c->Hp + kBinTile - 1) / kBinTile);
    ReconArgs a = recon_args(c, r);
    a.batch_t = b.bt_at(b_lo); a.nb = b_hi - b_lo;
    launch_recon_pose_table(a, b.pose_at(b_lo), c->stream);
    ReconLdsArgs g{};
    g.cam = a.cam;
    g.cam.poseR = b.pose_at(b_lo);
    g.cam.xy = b.xy_at(first);
    g.cam.per_batch = p.per_batch;
    g.cam.n = (int)n;
    g.cam.order = r->sup.order;
    const ChunkPlan cp = plan_chunks(n, 2 * tiles, kBackEndChunkDiv);
    int rc = b.ts.reserve(c, n, 2 * tiles, cp.max_chunks);
    if (!rc) rc = bound_sort(c, b, g.cam, cp.chunk_events);
    if (rc) return rc;
    b.sorted = false;
    g.ev.sxy = b.ts.d_sxy; g.ev.sbatch = b.ts.d_sbatch;
    g.ev.chunks = b.ts.d_chunks; g.ev.nchunks = (int)cp.max_chunks; g.ev.nchunks_dev = b.ts.d_nchunks;
    g.ev.fallback = b.ts.d_fallback;
    g.ev.fixed = r->deterministic ? static_cast<unsigned long long *>(d_base) : nullptr;
    g.plane = r->deterministic ? nullptr : static_cast<float *>(d_base);
    g.n_inside = d_inside;
    HIP_TRY(c, hipMemsetAsync(b.ts.d_fallback, 0, sizeof(unsigned), c->stream));
    launch_recon_votes_lds(g, c->stream);
  }
  HIP_TRY(c, hipGetLastError());
  return CMX_OK;
}
// the active part's chunk table: the chunk rule at ITS count (the table may be longer than the one the bind reserved)
static int frozen_plan_active(cmx_ctx *c, ReconState *r, ReconFrozen *fz) {
  const int64_t n_act = r->bnd.plan.n_packed - fz->sampled;
  if (n_act <= 0) return CMX_OK;
  const int tiles = ((c->Wp + kBinTile - 1) / kBinTile) * ((c->Hp + kBinTile - 1) / kBinTile);
  const ChunkPlan cp = plan_chunks(n_act, 2 * tiles, kBackEndChunkDiv);
  fz->chunk_events = cp.chunk_events;
  fz->max_chunks = (int)cp.max_chunks;
  return r->bnd.ts.reserve(c, n_act, 2 * tiles, cp.max_chunks);
}

int cmx_backend_recon_freeze_head(cmx_ctx *c, int num_fixed) {
  int rc = recon_enter(c, true);
  if (rc) return rc;
  ReconState *r = c->recon;
  if (!r->bound) return fail(c, CMX_ERR_STATE, "no events are bound (cmx_backend_recon_bind_from)");
  if (num_fixed < 0 || num_fixed >= r->sup.K) return fail(c, CMX_ERR_INVALID_ARG, "num_fixed=%d outside [0, %d)", num_fixed, r->sup.K);
  rc = recon_refuse_released(c, r, "freeze_head");
  if (rc) return rc;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  (void)recon_pass_enter(c, r, false);  // as a bind: an open gradient pass is closed
  frozen_drop(c, r);
  if (num_fixed == 0) return CMX_OK;
  ReconBound &b = r->bnd;
  const BatchPlan &p = b.plan;
  ReconFrozen fz;
  auto build = [&]() -> int {
    // the prefix rule on the host, over the binding's batch times read back once
    std::vector<long long> bt((size_t)p.nb);
    if (p.nb > 0) HIP_TRY(c, hipMemcpy(bt.data(), b.d_bt, (size_t)p.nb * sizeof(long long), hipMemcpyDeviceToHost));
    fz.b_act = frozen_prefix(r->sup, num_fixed, bt.data(), p.nb);
    fz.sampled = p.packed(0, fz.b_act);
    fz.knots.resize(4 * (size_t)num_fixed);
    HIP_TRY(c, hipMemcpy(fz.knots.data(), r->d_knots, (size_t)num_fixed * sizeof(Quat), hipMemcpyDeviceToHost));
    // the base: the frozen batches' votes at the current knots
    const size_t np = (size_t)c->Wp * c->Hp, cell = r->deterministic ? sizeof(unsigned long long) : sizeof(float);
    HIP_TRY(c, hipMalloc(&fz.d_base, np * cell));
    HIP_TRY(c, hipMalloc((void **)&fz.d_inside, sizeof(unsigned long long)));
    HIP_TRY(c, hipMemsetAsync(fz.d_base, 0, np * cell, c->stream));
    HIP_TRY(c, hipMemsetAsync(fz.d_inside, 0, sizeof(unsigned long long), c->stream));
    int rc2 = frozen_vote(c, r, fz.d_base, fz.d_inside, 0, fz.b_act);
    if (rc2) return rc2;
    HIP_TRY(c, hipMemcpyAsync(&fz.inside, fz.d_inside, sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    rc2 = frozen_plan_active(c, r, &fz);
    if (rc2) return rc2;
    fz.num_fixed = num_fixed;
    return CMX_OK;
  };
  rc = build();
  if (rc) {
    (void)hipStreamSynchronize(c->stream);
    fz.release();
    return rc;
  }
  r->frozen = fz;
  r->bnd.sorted = false;  // (the sort holds the active events alone from the next evaluation on)
  return CMX_OK;
}

int cmx_backend_recon_frozen_info(cmx_ctx *c, int *num_fixed, int64_t *frozen_batches, int64_t *frozen_sampled) {
  int rc = recon_enter(c, true);
  if (rc) return rc;
  const ReconFrozen &fz = c->recon->frozen;  // (without a frozen head: all zero)
  if (num_fixed) *num_fixed = fz.num_fixed;
  if (frozen_batches) *frozen_batches = fz.num_fixed ? fz.b_act : 0;
  if (frozen_sampled) *frozen_sampled = fz.num_fixed ? fz.sampled : 0;
  return CMX_OK;
}

// ---- a binding that grows
// The freeze line moves forward: the batches [b_act, b_act') the prefix rule newly names under num_fixed_new fixed knots vote once, at
// the knots the reconstruction holds, into the base as it stands.  Frozen batches read fixed knots alone, and those are bytewise the
// same at every evaluation and extend since the freeze, so the base is what one freeze of [0, b_act') would have voted.
int cmx_backend_recon_advance_head(cmx_ctx *c, int num_fixed_new) {
  int rc = recon_enter(c, true);
  if (rc) return rc;
  ReconState *r = c->recon;
  if (!r->bound) return fail(c, CMX_ERR_STATE, "no events are bound (cmx_backend_recon_bind_from)");
  ReconFrozen &fz = r->frozen;
  if (num_fixed_new < fz.num_fixed || num_fixed_new >= r->sup.K)
    return fail(c, CMX_ERR_INVALID_ARG, "num_fixed_new=%d outside [%d, %d)", num_fixed_new, fz.num_fixed, r->sup.K);
  if (fz.num_fixed == 0) return cmx_backend_recon_freeze_head(c, num_fixed_new);
  ReconBound &b = r->bnd;
  const BatchPlan &p = b.plan;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  // the prefix rule from the line on, over the active batches' times
  const int n_act_b = p.nb - fz.b_act;
  std::vector<long long> bt((size_t)n_act_b);
  if (n_act_b > 0) HIP_TRY(c, hipMemcpy(bt.data(), b.bt_at(fz.b_act), (size_t)n_act_b * sizeof(long long), hipMemcpyDeviceToHost));
  const int b_new = fz.b_act + frozen_prefix(r->sup, num_fixed_new, bt.data(), n_act_b);
  std::vector<double> knots(4 * (size_t)num_fixed_new);
  HIP_TRY(c, hipMemcpy(knots.data(), r->d_knots, (size_t)num_fixed_new * sizeof(Quat), hipMemcpyDeviceToHost));
  // from here on only a runtime error can end the call
  (void)recon_pass_enter(c, r, false);  // as freeze_head: an open gradient pass is closed
  rc = frozen_vote(c, r, fz.d_base, fz.d_inside, fz.b_act, b_new);
  if (!rc) {
    const hipError_t e = hipMemcpyAsync(&fz.inside, fz.d_inside, sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream);
    if (e != hipSuccess) rc = fail(c, CMX_ERR_HIP, "reading the base's counter: %s", hipGetErrorString(e));
  }
  const hipError_t waited = hipStreamSynchronize(c->stream);
  if (!rc && waited != hipSuccess) rc = fail(c, CMX_ERR_HIP, "the votes of the newly frozen batches failed: %s", hipGetErrorString(waited));
  if (rc) return rc;
  fz.b_act = b_new;
  fz.sampled = p.packed(0, b_new);
  fz.knots = knots;
  fz.num_fixed = num_fixed_new;
  b.sorted = false;  // (the sort holds the newly frozen events, or the old active ones)
  return frozen_plan_active(c, r, &fz);
}

// The frozen batches' resident entries go: the active tail moves into buffers of its own size and the old ones are freed, so the
// binding holds (and its capacity follows) the active tail, not the recording.  The open tail's raw events stay.
int cmx_backend_recon_release_head(cmx_ctx *c) {
  int rc = recon_enter(c, true);
  if (rc) return rc;
  ReconState *r = c->recon;
  if (!r->bound) return fail(c, CMX_ERR_STATE, "no events are bound (cmx_backend_recon_bind_from)");
  ReconBound &b = r->bnd;
  const ReconFrozen &fz = r->frozen;
  const BatchPlan &p = b.plan;
  if (fz.num_fixed == 0 || fz.b_act <= b.rel_batches) return CMX_OK;  // nothing (new) to give back
  // The released entries are dead space in front of the live ones.  Once there is more dead than live the live tail moves into
  // buffers of twice its size and the old ones are freed (a copy of `live` entries per more than `live` released: amortised, and
  // the capacity stays within twice the active tail); until then -- and an append that runs out of room does the same -- the
  // release is book-keeping alone.
  const size_t n_xy = (size_t)(p.n_packed - fz.sampled), n_bt = (size_t)(p.nb - fz.b_act);
  if ((size_t)(fz.sampled - b.base_sampled) > n_xy) {
    const size_t cap_xy = n_xy ? 2 * n_xy : 1, cap_bt = n_bt ? 2 * n_bt : 1;
    uint32_t *xy = nullptr;
    long long *bt = nullptr;
    PoseR *pose = nullptr;
    hipError_t e = hipStreamSynchronize(c->stream);
    if (e == hipSuccess) e = hipMalloc((void **)&xy, cap_xy * sizeof(uint32_t));
    if (e == hipSuccess) e = hipMalloc((void **)&bt, cap_bt * sizeof(long long));
    if (e == hipSuccess) e = hipMalloc((void **)&pose, cap_bt * sizeof(PoseR));
    if (e == hipSuccess && n_xy) e = hipMemcpyAsync(xy, b.xy_at(fz.sampled), n_xy * sizeof(uint32_t), hipMemcpyDeviceToDevice, c->stream);
    if (e == hipSuccess && n_bt) e = hipMemcpyAsync(bt, b.bt_at(fz.b_act), n_bt * sizeof(long long), hipMemcpyDeviceToDevice, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) {  // (the binding is as it was)
      (void)hipStreamSynchronize(c->stream);
      (void)hipFree(xy); (void)hipFree(bt); (void)hipFree(pose);
      return fail(c, CMX_ERR_HIP, "moving the active tail: %s", hipGetErrorString(e));
    }
    (void)hipFree(b.d_xy); (void)hipFree(b.d_bt); (void)hipFree(b.d_poseR);
    b.d_xy = xy; b.d_bt = bt; b.d_poseR = pose;
    b.xy_cap = cap_xy;
    b.bt_cap = cap_bt;
    b.base_sampled = fz.sampled;
    b.base_batches = fz.b_act;
  }
  b.rel_batches = fz.b_act;
  b.rel_sampled = fz.sampled;
  // (whole batches in front of an active one; all of them: every event a batch holds -- a lone trailing event is in none)
  b.rel_events = fz.b_act < p.nb ? (int64_t)fz.b_act * p.B : (int64_t)(p.nb - 1) * p.B + p.last_len;
  return CMX_OK;
}

int cmx_backend_recon_online_info(cmx_ctx *c, int64_t *released_batches, int64_t *released_events, int64_t *released_sampled,
                                  int64_t *resident_sampled) {
  int rc = recon_enter(c, true);
  if (rc) return rc;
  const ReconState *r = c->recon;  // (without a binding: all zero)
  if (released_batches) *released_batches = r->bound ? r->bnd.rel_batches : 0;
  if (released_events) *released_events = r->bound ? r->bnd.rel_events : 0;
  if (released_sampled) *released_sampled = r->bound ? r->bnd.rel_sampled : 0;
  if (resident_sampled) *resident_sampled = r->bound ? r->bnd.resident_sampled() : 0;
  return CMX_OK;
}

// `count` events behind the bound ones: the binding afterwards is bind_from's over the concatenation.  plan_append (cmx_ingest.hpp)
// names the batch that is cut again; "the kept open tail ++ the new range" is assembled in a scratch of count + B events at most, and
// the batch-time and packing kernels of bind_from run over that scratch alone.
int cmx_backend_recon_bind_append_from(cmx_ctx *c, const cmx_events *e, int64_t first, int64_t count) {
  int rc = recon_enter(c, true);
  if (rc) return rc;
  ReconState *r = c->recon;
  if (!r->bound) return fail(c, CMX_ERR_STATE, "no events are bound (cmx_backend_recon_bind_from)");
  EventSource src;
  rc = store_source(c, e, first, count, &src);
  if (rc) return rc;
  (void)recon_pass_enter(c, r, false);  // as every add: an open gradient pass is closed
  if (src.n > kMaxEvents) return fail(c, CMX_ERR_INVALID_ARG, "bad event count %lld", (long long)src.n);
  if (src.n == 0) return CMX_OK;
  ReconBound &b = r->bnd;
  ReconFrozen &fz = r->frozen;
  if (b.n_events > 0 && (long long)src.soa.t[0] < b.t_last)
    return fail(c, CMX_ERR_TIME_ORDER, "the first new event (%lld ns) is earlier than the last bound one (%lld ns)", (long long)src.soa.t[0],
                b.t_last);
  AppendPlan ap;
  if (!plan_append(b.n_events, src.n, r->B, r->rate, &ap)) return fail(c, CMX_ERR_INVALID_ARG, "too many batches");
  if (fz.num_fixed > 0 && ap.b_recut < fz.b_act)
    return fail(c, CMX_ERR_STATE, "batch %d, which the new events cut again, is part of the frozen head (%d batches)", ap.b_recut, fz.b_act);
  if (ap.plan.n_packed - b.rel_sampled > kMaxBoundSampled)
    return fail(c, CMX_ERR_INVALID_ARG, "%lld resident sampled events above the limit of a binding (2^30)",
                (long long)(ap.plan.n_packed - b.rel_sampled));
  if (ap.tail_n != b.tail_n) return fail(c, CMX_ERR_STATE, "the binding's open tail holds %lld events, its plan says %lld", (long long)b.tail_n,
                                         (long long)ap.tail_n);
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  // ---- the scratch stream and its batch times (staging: nothing of the binding is touched)
  const int64_t m = ap.tail_n + src.n;
  if ((size_t)m > r->app_cap) {
    (void)hipFree(r->d_app_xy); (void)hipFree(r->d_app_t);
    r->d_app_xy = nullptr; r->d_app_t = nullptr; r->app_cap = 0;
    const size_t cap = (size_t)m + (size_t)m / 2;
    HIP_TRY(c, hipMalloc((void **)&r->d_app_xy, cap * sizeof(uint32_t)));
    HIP_TRY(c, hipMalloc((void **)&r->d_app_t, cap * sizeof(int64_t)));
    r->app_cap = cap;
  }
  if (ap.tail_n > 0) {
    HIP_TRY(c, hipMemcpyAsync(r->d_app_xy, b.d_tail_xy, (size_t)ap.tail_n * sizeof(uint32_t), hipMemcpyDeviceToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(r->d_app_t, b.d_tail_t, (size_t)ap.tail_n * sizeof(int64_t), hipMemcpyDeviceToDevice, c->stream));
  }
  HIP_TRY(c, hipMemcpyAsync(r->d_app_xy + ap.tail_n, src.d_xy, (size_t)src.n * sizeof(uint32_t), hipMemcpyDeviceToDevice, c->stream));
  HIP_TRY(c, hipMemcpyAsync(r->d_app_t + ap.tail_n, src.d_t, (size_t)src.n * sizeof(int64_t), hipMemcpyDeviceToDevice, c->stream));
  const BatchPlan &sp = ap.scratch;
  ReconSlot &s = r->slot[0];
  if (sp.nb > 0) {
    rc = slot_ensure(c, s, 0, (size_t)sp.nb, false);
    if (rc) return rc;
    rc = queue_batch_times(c, r->d_app_t, m, r->B, sp.nb, r->sup, s.d_bt, r->d_err, true);
    if (rc) return rc;
    HIP_TRY(c, hipGetLastError());
    BatchTimeError bad;
    rc = read_batch_errors(c, r->d_err, &bad);
    if (rc) return rc;
    if (bad.kind) return fail_batch_time(c, bad, r->sup, /*with_event=*/false);
  }
  // ---- valid.  Room for the longer binding, beside the buffers in use, when the arrays' end is reached: twice the LIVE entries (so
  // dead space in front, left by release_head, is dropped on the way and the capacity follows the active tail), the live part
  // copied across; a failure frees the new buffers alone
  const int tiles = ((c->Wp + kBinTile - 1) / kBinTile) * ((c->Hp + kBinTile - 1) / kBinTile);
  const int64_t n_act = ap.plan.n_packed - (fz.num_fixed > 0 ? fz.sampled : 0);
  const ChunkPlan cp = plan_chunks(n_act > 0 ? n_act : 1, 2 * tiles, kBackEndChunkDiv);
  const size_t need_xy = (size_t)(ap.plan.n_packed - b.rel_sampled), need_bt = (size_t)(ap.plan.nb - b.rel_batches);
  const size_t keep_xy = (size_t)(ap.packed_at - b.rel_sampled), keep_bt = (size_t)(ap.b_recut - b.rel_batches);
  const int64_t tail_from = open_tail_from(b.n_events + src.n, ap.plan), tail_new = b.n_events + src.n - tail_from;  // the next open tail
  uint32_t *xy = nullptr, *tail_xy = nullptr;
  long long *bt = nullptr;
  PoseR *pose = nullptr;
  int64_t *tail_t = nullptr;
  size_t xy_cap = b.xy_cap, bt_cap = b.bt_cap, tail_cap = b.tail_cap;
  hipError_t he = hipSuccess;
  if ((size_t)(ap.plan.n_packed - b.base_sampled) > b.xy_cap) {
    xy_cap = 2 * need_xy;
    he = hipMalloc((void **)&xy, xy_cap * sizeof(uint32_t));
    if (he == hipSuccess && keep_xy) he = hipMemcpyAsync(xy, b.xy_at(b.rel_sampled), keep_xy * sizeof(uint32_t), hipMemcpyDeviceToDevice, c->stream);
  }
  if (he == hipSuccess && (size_t)(ap.plan.nb - b.base_batches) > b.bt_cap) {
    bt_cap = 2 * need_bt;
    he = hipMalloc((void **)&bt, bt_cap * sizeof(long long));
    if (he == hipSuccess) he = hipMalloc((void **)&pose, bt_cap * sizeof(PoseR));
    if (he == hipSuccess && keep_bt) he = hipMemcpyAsync(bt, b.bt_at(b.rel_batches), keep_bt * sizeof(long long), hipMemcpyDeviceToDevice, c->stream);
  }
  if (he == hipSuccess && (size_t)tail_new > b.tail_cap) {
    tail_cap = (size_t)tail_new > 2 * b.tail_cap ? (size_t)tail_new : 2 * b.tail_cap;
    he = hipMalloc((void **)&tail_xy, tail_cap * sizeof(uint32_t));
    if (he == hipSuccess) he = hipMalloc((void **)&tail_t, tail_cap * sizeof(int64_t));
  }
  if (he == hipSuccess) he = hipStreamSynchronize(c->stream);
  rc = he == hipSuccess ? (n_act > 0 ? b.ts.reserve(c, n_act, 2 * tiles, cp.max_chunks) : (int)CMX_OK)
                        : fail(c, CMX_ERR_HIP, "growing the binding: %s", hipGetErrorString(he));
  if (rc) {  // (the binding is as it was)
    (void)hipStreamSynchronize(c->stream);
    (void)hipFree(xy); (void)hipFree(bt); (void)hipFree(pose); (void)hipFree(tail_xy); (void)hipFree(tail_t);
    return rc;
  }
  // ---- commit: from here on only a runtime error can end the call
  if (xy) { (void)hipFree(b.d_xy); b.d_xy = xy; b.xy_cap = xy_cap; b.base_sampled = b.rel_sampled; }
  if (bt) { (void)hipFree(b.d_bt); (void)hipFree(b.d_poseR); b.d_bt = bt; b.d_poseR = pose; b.bt_cap = bt_cap; b.base_batches = b.rel_batches; }
  if (tail_xy) { (void)hipFree(b.d_tail_xy); (void)hipFree(b.d_tail_t); b.d_tail_xy = tail_xy; b.d_tail_t = tail_t; b.tail_cap = tail_cap; }
  b.n_events += src.n;
  b.plan = ap.plan;
  b.t_last = (long long)src.soa.t[src.n - 1];
  b.sorted = false;
  if (n_act > 0) {  // the chunk rule at the new (active) count
    if (fz.num_fixed > 0) { fz.chunk_events = cp.chunk_events; fz.max_chunks = (int)cp.max_chunks; }
    else { b.chunk_events = cp.chunk_events; b.max_chunks = (int)cp.max_chunks; }
  }
  if (sp.nb > 0) {
    HIP_TRY(c, hipMemcpyAsync(b.bt_at(ap.b_recut), s.d_bt, (size_t)sp.nb * sizeof(long long), hipMemcpyDeviceToDevice, c->stream));
    // (t_next = the smallest time: no event carries the old flag)
    launch_be_pack_from_store(r->d_app_xy, reinterpret_cast<const long long *>(r->d_app_t), (long long)m, r->B, r->rate, sp.per_batch,
                              (int)sp.n_packed, std::numeric_limits<long long>::min(), b.xy_at(ap.packed_at), c->stream);
    HIP_TRY(c, hipGetLastError());
  }
  rc = tail_keep(c, &b, r->d_app_xy + (tail_from - ap.keep_from), r->d_app_t + (tail_from - ap.keep_from), tail_new);
  if (rc) return rc;
  HIP_TRY(c, hipStreamSynchronize(c->stream));  // the store may be pushed to, compacted or closed from here on
  return CMX_OK;
}

// ---- cmx_backend_recon_solve's three hooks (the FR-CG loop itself is cmx_solver.cpp's)
// begin: every argument error, before anything changes; then the staging, the start knots on the device and -- asked for -- the
// frozen head at them
int recon_solve_begin(cmx_ctx *c, const double *knots_xyzw, int num_fixed, int freeze_head, double blur_sigma, int contrast_measure,
                      int *n_params) {
  int rc = recon_enter(c, true);
  if (rc) return rc;
  ReconState *r = c->recon;
  if (!r->bound) return fail(c, CMX_ERR_STATE, "no events are bound (cmx_backend_recon_bind_from)");
  if (!knots_xyzw) return fail(c, CMX_ERR_INVALID_ARG, "null knot array");
  const int K = r->sup.K;
  if (num_fixed < 0 || num_fixed >= K) return fail(c, CMX_ERR_INVALID_ARG, "num_fixed=%d outside [0, %d)", num_fixed, K);
  if (!std::isfinite(blur_sigma)) return fail(c, CMX_ERR_INVALID_ARG, "blur_sigma is not finite");
  const bool keep = freeze_head == CMX_RECON_KEEP_HEAD;
  if (keep) {  // under the frozen head as it stands
    const ReconFrozen &fz = r->frozen;
    if (fz.num_fixed == 0) return fail(c, CMX_ERR_STATE, "no frozen head to keep (cmx_backend_recon_freeze_head / _advance_head)");
    if (num_fixed != fz.num_fixed) return fail(c, CMX_ERR_INVALID_ARG, "num_fixed=%d, the frozen head has %d", num_fixed, fz.num_fixed);
    if (memcmp(knots_xyzw, fz.knots.data(), (size_t)fz.num_fixed * sizeof(Quat)) != 0)
      return fail(c, CMX_ERR_INVALID_ARG, "the first %d knots differ from those the head was frozen at", fz.num_fixed);
  } else {
    rc = recon_refuse_released(c, r, "a solve that freezes again or drops the head");
    if (rc) return rc;
  }
  rc = recon_grad_precheck(c, r, blur_sigma);
  if (rc) return rc;
  ReconSolve &sv = r->solve;
  if (!sv.h_knots) {
    HIP_TRY(c, hipHostMalloc((void **)&sv.h_knots, (size_t)K * sizeof(Quat), hipHostMallocDefault));
    HIP_TRY(c, hipHostMalloc((void **)&sv.h_cm, 2 * sizeof(double), hipHostMallocDefault));
    HIP_TRY(c, hipHostMalloc((void **)&sv.h_cnt, 2 * sizeof(unsigned long long), hipHostMallocDefault));
    HIP_TRY(c, hipHostMalloc((void **)&sv.h_grad, 3 * (size_t)K * sizeof(double), hipHostMallocMapped));
    HIP_TRY(c, hipHostGetDevicePointer((void **)&sv.d_grad, sv.h_grad, 0));
  }
  sv.k0.assign(knots_xyzw, knots_xyzw + 4 * (size_t)K);
  sv.num_fixed = num_fixed;
  sv.sigma = blur_sigma;
  sv.measure = contrast_measure;
  sv.have_last = false;
  sv.evals = 0;
  sv.waits = 0;
  if (keep) {  // the start knots by extend's path: the head survives
    rc = cmx_backend_recon_extend(c, K, knots_xyzw);
  } else if (freeze_head) {  // at the start knots: they go to the device first (restart, which also drops an earlier head)
    rc = cmx_backend_recon_restart(c, knots_xyzw);
    if (!rc) rc = cmx_backend_recon_freeze_head(c, num_fixed);
  } else {  // every event, every time
    rc = cmx_backend_recon_freeze_head(c, 0);
  }
  if (rc) return rc;
  *n_params = 3 * (K - num_fixed);
  return CMX_OK;
}

// the knots of increment x: the start knots moved by cmx_traj_incremental_update itself, into the pinned staging
static void solve_moved(const ReconState *r, const ReconSolve &sv, const double *x, double *knots) {
  const int K = r->sup.K;
  memcpy(knots, sv.k0.data(), (size_t)K * sizeof(Quat));
  (void)cmx_traj_incremental_update(K, knots, sv.num_fixed, 3 * (K - sv.num_fixed), x);
}

int recon_solve_eval(cmx_ctx *c, const double *x, double *contrast, double *grad_free) {
  ReconState *r = c->recon;
  ReconSolve &sv = r->solve;
  solve_moved(r, sv, x, sv.h_knots);
  const int64_t w0 = r->host_waits;
  const int rc = bound_eval(c, r, sv.h_knots, sv.sigma, sv.measure, contrast, grad_free, &sv);
  sv.evals++;
  sv.waits += r->host_waits - w0;
  const size_t n = 3 * (size_t)(r->sup.K - sv.num_fixed);
  sv.last_x.assign(x, x + n);
  sv.have_last = rc == CMX_OK;
  return rc;
}

// end: the refined knots to the caller, and the reconstruction at their evaluation -- one more cost-only evaluation when the last
// trial point was another one
int recon_solve_end(cmx_ctx *c, const double *x, double *knots_out) {
  ReconState *r = c->recon;
  ReconSolve &sv = r->solve;
  const size_t n = 3 * (size_t)(r->sup.K - sv.num_fixed);
  int rc = CMX_OK;
  if (!sv.have_last || memcmp(sv.last_x.data(), x, n * sizeof(double)) != 0) {
    double con = 0;
    rc = recon_solve_eval(c, x, &con, nullptr);
  }
  solve_moved(r, sv, x, knots_out);
  return rc;
}

int cmx_diag_recon_solve_counts(cmx_ctx *c, int64_t *evaluations, int64_t *host_waits) {
  int rc = recon_enter(c, true);
  if (rc) return rc;
  if (evaluations) *evaluations = c->recon->solve.evals;
  if (host_waits) *host_waits = c->recon->solve.waits;
  return CMX_OK;
}

// the plane as fp32 on the device: in deterministic mode the current fixed-point sums, converted (they stay: votes may follow)
static void recon_refresh_plane(cmx_ctx *c, ReconState *r) {
  if (r->deterministic) launch_recon_fixed_to_float(r->d_fixed, r->d_plane, (size_t)c->Wp * c->Hp, c->stream);
}

int cmx_backend_recon_get(cmx_ctx *c, float *pano, int64_t *n_sampled, int64_t *n_inside) {
  int rc = recon_enter(c, true);
  if (rc) return rc;
  ReconState *r = c->recon;
  unsigned long long inside = 0;
  if (pano) {
    recon_refresh_plane(c, r);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(pano, r->d_plane, (size_t)c->Wp * c->Hp * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  }
  if (n_inside) HIP_TRY(c, hipMemcpyAsync(&inside, r->d_inside, sizeof(inside), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  if (n_sampled) *n_sampled = r->n_sampled;
  if (n_inside) *n_inside = (int64_t)inside;
  return CMX_OK;
}

// cmx_backend_render_map's tone map (PoseGraphOptimizer::publishEventImage, pose_graph_optimizer.cpp:378-413) on the reconstruction
int cmx_backend_recon_render(cmx_ctx *c, double gamma, const double fov_quat_xyzw[4], unsigned char *out) {
  int rc = recon_enter(c, true);
  if (rc) return rc;
  if (!out) return fail(c, CMX_ERR_INVALID_ARG, "null output buffer");
  if (!std::isfinite(gamma) || !(gamma > 0.0)) return fail(c, CMX_ERR_INVALID_ARG, "gamma must be finite and > 0");
  Quat q{0, 0, 0, 1};
  if (fov_quat_xyzw) {
    const double *v = fov_quat_xyzw;
    const double nrm = sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2] + v[3] * v[3]);
    if (!std::isfinite(nrm) || !(nrm > 0.0)) return fail(c, CMX_ERR_INVALID_ARG, "pose quaternion has no direction");
    q = Quat{v[0] / nrm, v[1] / nrm, v[2] / nrm, v[3] / nrm};
  }
  ReconState *r = c->recon;
  const size_t np = (size_t)c->Wp * c->Hp, bytes = fov_quat_xyzw ? 3 * np : np;
  rc = display_begin(c, bytes);
  if (rc) return rc;
  recon_refresh_plane(c, r);
  launch_display_range(r->d_plane, nullptr, np, c->d_disp_range, c->stream);
  launch_display_map(r->d_plane, np, (float)gamma, fov_quat_xyzw != nullptr, c->d_disp_range, c->d_disp, c->stream);
  if (fov_quat_xyzw) {
    const Mat3 R = q_to_R(q);
    launch_display_fov(be_args(c), R.m, c->H, c->d_disp, c->stream);
  }
  return display_deliver(c, bytes, out);
}
