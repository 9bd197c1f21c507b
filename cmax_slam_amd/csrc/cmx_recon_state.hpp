// cmx_recon_state.hpp -- what the three sources of cmx_backend_recon_* share: the state a reconstruction keeps (cmx_ctx::recon) and
// the helpers every one of them goes through.
//   cmx_reconstruct.cpp  life cycle (begin, restart, extend, end), contrast / grad_get / eval_from, get / render, and the three target
//                        sets (views, voxel grids, time surfaces) through ONE ReconTargetSet: begin, reset, end, get*, render, decay
//   cmx_recon_feed.cpp   one walk over the events handed in, in slices of whole batches: add*, grad_add*, warp*, pol_add*, and
//                        view_add* / voxel_add* / surface_add* through one recon_set_add_source
//   cmx_recon_bound.cpp  events bound once and evaluated many times: bind / eval_bound, the frozen head, append / advance /
//                        release, the hooks of cmx_backend_recon_solve
// Kernels: cmx_recon.hip.
#pragma once
#include "cmx_context.hpp"

// A slice holds at most max(slice size, one batch) packed events, and the vote kernel indexes a slice with ints: both are
// kept at or below 2^30, far from the wrap.
constexpr int kMaxSliceEvents = 1 << 30;

// Input staging of one slice.  The host paths hold packed events and batch times (voxel_add*, surface_add*: and the packed events' own timestamps)
// in pinned memory and on the device; the store
// paths read the store's events in place and form the batch times on the device, so they use slot[0]'s device table alone.
struct ReconSlot {
  uint32_t *h_xy = nullptr, *d_xy = nullptr;
  long long *h_bt = nullptr, *d_bt = nullptr;
  int64_t *h_t = nullptr, *d_t = nullptr;  // the packed events' own timestamps, beside the words (voxel_add*, surface_add*)
  size_t h_xy_cap = 0, xy_cap = 0, h_bt_cap = 0, bt_cap = 0, h_t_cap = 0, t_cap = 0;
  hipEvent_t up = nullptr, done = nullptr;  // upload complete (copy stream) / the slice's kernels complete (context stream)
  bool busy = false;
  void release() {
    if (h_xy) (void)hipHostFree(h_xy);
    if (h_bt) (void)hipHostFree(h_bt);
    if (h_t) (void)hipHostFree(h_t);
    (void)hipFree(d_xy);
    (void)hipFree(d_bt);
    (void)hipFree(d_t);
    if (up) (void)hipEventDestroy(up);
    if (done) (void)hipEventDestroy(done);
    *this = ReconSlot{};
  }
};

// Output staging of the per-event export (cmx_backend_recon_warp*, host output): the kernel of slice k writes into d_*, a copy on the
// download stream moves it into pinned h_*, and the host pool copies it into the caller's arrays while slice k+1 runs.
struct ReconWarpSlot {
  double *d_xy = nullptr, *h_xy = nullptr;  // two per event (16 bytes of coordinates each, the wider format)
  unsigned char *d_fl = nullptr, *h_fl = nullptr;
  size_t d_xy_cap = 0, h_xy_cap = 0, d_fl_cap = 0, h_fl_cap = 0;
  hipEvent_t kdone = nullptr, down = nullptr;  // kernel complete (context stream) / download complete (download stream)
  void release() {
    if (h_xy) (void)hipHostFree(h_xy);
    if (h_fl) (void)hipHostFree(h_fl);
    (void)hipFree(d_xy);
    (void)hipFree(d_fl);
    if (kdone) (void)hipEventDestroy(kdone);
    if (down) (void)hipEventDestroy(down);
    *this = ReconWarpSlot{};
  }
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

typedef double ReconRows[2 * 3 * kReconWindow];  // one row of window sums (ReconGatherArgs::rows)

// One set of vote targets beside the panorama -- pinhole views, voxel grids or time surfaces: n virtual cameras
// with a time range each, and what their votes land in.  The reconstruction's own: made by cmx_backend_recon_<api>_begin, cleared
// by restart and _reset, freed by _end, begin and end; nothing but <api>_add* writes it and nothing but <api>_get* / render /
// decay reads it.
struct ReconTargetSet {
  const char *noun, *api;                      // "view" / "grid" / "surface" in the error texts; the <api> of the calls' names
  bool timestamps;                             // the targets hold int64 timestamps (d_cells), not vote sums (d_planes, d_fixed)
  int n = 0, W = 0, H = 0;                     // n == 0: no set
  int per = 1;                                 // planes of W x H per target: 1 (views), n_bins (grids), channels (surfaces)
  bool polarity = false;                       // a signed voxel set / a by-polarity surface set: the events' polarity is read
  void *d_entries = nullptr;                   // [n] ReconViewDev (views, surfaces) or ReconVoxelDev; says whether the set exists
  ReconViewRange *d_ranges = nullptr;          // [n] the time ranges alone: what a vote workgroup scans
  float *d_planes = nullptr;                   // [n][per][H * W] (default mode), or the fp32 view of d_fixed made by get / render
  unsigned long long *d_fixed = nullptr;       // deterministic mode: their 2^-30 fixed-point twins (voxel grids: two's complement)
  long long *d_cells = nullptr;                // [n][per][H * W] the latest timestamp voted into each cell, or INT64_MIN
  unsigned long long *d_voted = nullptr;       // [n] events that voted into each target
  size_t cells_per_target() const { return (size_t)per * W * H; }
  void release() {
    void *dev[] = {d_entries, d_ranges, d_planes, d_fixed, d_cells, d_voted};
    for (void *p : dev) (void)hipFree(p);
    *this = ReconTargetSet{noun, api, timestamps};
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
  ReconRows *d_rows = nullptr;            // deterministic mode: one row of window sums per gather workgroup of a slice ...
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
  // ---- signed polarity map (cmx_backend_recon_pol_*): two planes of the reconstruction's own beside the count plane,
  // allocated by the first pol_add*, cleared by restart and pol_reset, freed by end; nothing else reads or writes them
  float *d_pol = nullptr;                      // [2][Hp * Wp] ON then OFF (default mode), or the fp32 view of d_pol_fixed made by pol_get / pol_render
  unsigned long long *d_pol_fixed = nullptr;   // deterministic mode: their 2^-30 fixed-point twins
  unsigned long long *d_pol_inside = nullptr;  // [2] events that voted into the ON / the OFF plane
  // ---- target sets: pinhole views (cmx_backend_recon_view_*), voxel grids (_voxel_*), time surfaces (_surface_*)
  ReconTargetSet views{"view", "view", false}, voxels{"grid", "voxel", false}, surfaces{"surface", "surface", true};
  // the surface set's own, for surface_decay: freed with it
  long long *d_stref = nullptr;                // [surfaces.n] the reference times of a call that names them
  float *d_sdecay = nullptr;                   // (host output) the decayed cells on their way out, grown on demand
  size_t sdecay_cap = 0;
  // ---- per-event support scores (cmx_backend_recon_score*): open from score_open until something changes the plane or
  // the knots (recon_pass_enter, recon_start_over).  The taps are the pass's own copy: a contrast at another sigma rebuilds those
  // above and leaves the pass open.
  bool score_open = false;
  int score_radius = 0;                        // 0: S is the count plane itself (d_plane, refreshed by score_open)
  float score_taps[2 * kMaxRadius + 1] = {1.f};
  float *d_support = nullptr;                  // [Hp * Wp] S = G plane, allocated at the first score_open with sigma > 0
  int64_t host_waits = 0;               // times a host thread has waited for the device in this reconstruction's calls
  // everything above that owns memory, a stream or an event (the streams idle: recon_release has waited for them)
  void release() {
    if (copy_stream) (void)hipStreamDestroy(copy_stream);
    if (down_stream) (void)hipStreamDestroy(down_stream);
    for (ReconSlot &s : slot) s.release();
    for (ReconWarpSlot &s : wslot) s.release();
    void *dev[] = {d_knots, d_delta, d_plane, d_fixed, d_inside, d_err, d_cx, d_cy, d_tflags, d_tile_list, d_tile_count, d_partials,
                   d_cm, d_jt, d_gsum, d_voted, d_rows, d_row_win, d_app_xy, d_app_t, d_pol, d_pol_fixed, d_pol_inside, d_stref, d_sdecay,
                   d_support};
    for (void *p : dev) (void)hipFree(p);
    for (ReconTargetSet *t : {&views, &voxels, &surfaces}) t->release();
    bnd.release();
    frozen.release();
    solve.release();
  }
};

// sort tiles of the panorama (the binding's TileSort is reserved for twice as many keys: the back end's keys carry the old / new bit)
inline int recon_sort_tiles(const cmx_ctx *c) { return ((c->Wp + kBinTile - 1) / kBinTile) * ((c->Hp + kBinTile - 1) / kBinTile); }

// ---- cmx_reconstruct.cpp
// common front door: a plain back-end context (a group's handle has no reconstruction: CMX_ERR_STATE), bound to its device
int recon_enter(cmx_ctx *c, bool need_begun);
// every place one of these calls blocks on the stream goes through here (cmx_backend_recon_solve reports the count per evaluation)
hipError_t recon_wait(cmx_ctx *c, ReconState *r);
// batches of a call (plan_batches) and batches per slice (CMX_DIAG_RECON_SLICE_EVENTS)
int recon_slice_batches(const ReconState *r);
int recon_plan(cmx_ctx *c, const ReconState *r, int64_t n, BatchPlan *p, int *slice_batches);
ReconArgs recon_args(const cmx_ctx *c, const ReconState *r);
// the gradient pass's view of the same launch: the events and the spline of recon_args, Jt and the border factors, the sums
ReconGatherArgs recon_gather_args(const cmx_ctx *c, const ReconState *r);
// first thing of every pass over events: a vote pass closes an open gradient pass (and an open score pass), a gradient pass needs one
int recon_pass_enter(cmx_ctx *c, ReconState *r, bool grad);
// the front door of score*: recon_enter, and a score pass is open
int recon_score_enter(cmx_ctx *c);
// knot values for the trajectory of begin; plane, counters and gradient state start over (from_base: from the frozen head's votes;
// staged: the knots are in pinned memory that stays untouched until the caller's own wait)
int recon_start_over(cmx_ctx *c, ReconState *r, const double *knots_xyzw, bool from_base = false, bool staged = false);
// the binding changes, goes, or the knots are set anew: no frozen head any more, and the next evaluation sorts all events again
void frozen_drop(cmx_ctx *c, ReconState *r);
// events of the binding have been released: whatever would drop or rebuild the frozen base -- and keep the binding -- is refused
int recon_refuse_released(cmx_ctx *c, const ReconState *r, const char *what);
// the image pass over the plane, queued: contrast and mean on their way into cm[2]; with want_grad the gradient pass is open
int recon_contrast_queue(cmx_ctx *c, ReconState *r, double blur_sigma, int contrast_measure, int want_grad, double *cm);
// taps and border factors for this sigma, and the one argument error a gradient at it can find
int recon_grad_precheck(cmx_ctx *c, ReconState *r, double sigma);
// the polarity planes and their two counters: allocated (and zeroed) at the first pol_add*; zeroed, where they exist (queued)
int recon_pol_ensure(cmx_ctx *c, ReconState *r);
int recon_pol_clear(cmx_ctx *c, ReconState *r);
// a target set's planes (or cells: back to INT64_MIN) and its counters cleared, where the set exists (queued)
int recon_set_clear(cmx_ctx *c, ReconTargetSet *t);
// the front door of every call that needs the set: recon_enter, and the set's _begin has succeeded
int recon_set_enter(cmx_ctx *c, ReconTargetSet ReconState::*which);

// ---- cmx_recon_feed.cpp
// one slice of the gradient pass, as g.ev describes it; deterministic mode: the workgroups' rows, then their sum in workgroup order
int queue_gather(cmx_ctx *c, ReconState *r, ReconGatherArgs &g);
// batch times of events on the device over the whole range, slice by slice into d_bt (one slice's table), and their validation: the
// error words are read before anything of the call is queued behind them
int validate_store_times(cmx_ctx *c, ReconState *r, const int64_t *d_t, int64_t n, const BatchPlan &p, int slice_batches, long long *d_bt);
// the vote pass (or, grad, the gradient pass) of recon_add_from / recon_grad_add_from over a range of an event store
int recon_add_source(cmx_ctx *c, const EventSource &src, bool grad);
