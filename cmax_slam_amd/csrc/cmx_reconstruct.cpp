// cmx_reconstruct.cpp -- cmx_backend_recon_*: the panorama of ALL events warped along the FINAL trajectory, for a spline of any knot
// count.  One call of recon_add* is the vote loop of EventWarper::computeImageOfWarpedEvents (event_pano_warper.cpp:188-196,
// :233-311) over exactly the events handed in, added into a plane that belongs to the reconstruction alone: no old / new split, no
// alpha, no IG, no blur, and nothing of the window state, the resident evaluation point, the map or the exchange sets is touched.
// Kernels: cmx_recon.hip.
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
};

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
  (void)hipFree(r->d_knots);
  (void)hipFree(r->d_delta);
  (void)hipFree(r->d_plane);
  (void)hipFree(r->d_fixed);
  (void)hipFree(r->d_inside);
  (void)hipFree(r->d_err);
  delete r;
  c->recon = nullptr;
}

// common front door: a plain back-end context (a group's handle has no reconstruction: CMX_ERR_STATE), bound to its device
int recon_enter(cmx_ctx *c, bool need_begun) {
  if (!c || c->kind != KIND_BE) return fail(c, CMX_ERR_STATE, "not a back-end context");
  if (c->group) return fail(c, CMX_ERR_STATE, "reconstruction is not available on a group handle");
  if (need_begun && !c->recon) return fail(c, CMX_ERR_STATE, "cmx_backend_recon_begin has not succeeded");
  return bind_device(c);
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
  HIP_TRY(c, hipMemsetAsync(r->d_plane, 0, np * sizeof(float), c->stream));
  HIP_TRY(c, hipMemsetAsync(r->d_inside, 0, sizeof(unsigned long long), c->stream));
  if (r->deterministic) {
    HIP_TRY(c, hipMalloc((void **)&r->d_fixed, np * sizeof(unsigned long long)));
    HIP_TRY(c, hipMemsetAsync(r->d_fixed, 0, np * sizeof(unsigned long long), c->stream));
  }
  static_assert(sizeof(Quat) == 4 * sizeof(double), "knots travel as (x, y, z, w) doubles");
  HIP_TRY(c, hipMemcpyAsync(r->d_knots, knots_xyzw, (size_t)K * sizeof(Quat), hipMemcpyHostToDevice, c->stream));
  launch_recon_delta(r->d_knots, K, r->d_delta, c->stream);
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipStreamSynchronize(c->stream));  // the caller's knot array is free again
  return CMX_OK;
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
static int recon_plan(cmx_ctx *c, const ReconState *r, int64_t n, BatchPlan *p, int *slice_batches) {
  if (!plan_batches(n, r->B, r->rate, p)) return fail(c, CMX_ERR_INVALID_ARG, "too many batches");
  const int64_t sb = g_slice_events.load(std::memory_order_relaxed) / r->B;
  *slice_batches = (int)(sb < 1 ? 1 : sb);
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
int recon_add_host(cmx_ctx *c, const EventSource &src) {
  ReconState *r = c->recon;
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
  ReconArgs a = recon_args(c, r);
  // From here on only a runtime error (CMX_ERR_HIP) can end the call, and slices queued before it have voted: "a call that fails
  // adds nothing" is the contract of the validation above.  The slots are left idle either way.
  auto vote_slices = [&]() -> int {
  int k = 0;
  for (int b_lo = 0; b_lo < p.nb; b_lo += slice_batches, k++) {
    const int b_hi = (p.nb - b_lo > slice_batches) ? b_lo + slice_batches : p.nb;
    const int nbs = b_hi - b_lo;
    const int64_t ev_off = (int64_t)b_lo * B, np_s = p.packed(b_lo, b_hi);
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
    launch_recon_votes(a, c->stream);
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
  r->n_sampled += p.n_packed;
  return CMX_OK;
}

// events already on the device (event store): batch times and their validation by launch_be_batch_times, slice by slice into
// one slice-sized table; the error words are read before the first vote kernel of the call is queued
int recon_add_store(cmx_ctx *c, const EventSource &src) {
  ReconState *r = c->recon;
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
  auto slice_times = [&](int b_lo, int b_hi, bool clear_err) {
    const int64_t ev_off = (int64_t)b_lo * B;
    const int64_t n_s = b_hi == p.nb ? n - ev_off : (int64_t)(b_hi - b_lo) * B;
    return queue_batch_times(c, src.d_t + ev_off, n_s, B, b_hi - b_lo, r->sup, s.d_bt, r->d_err, clear_err);
  };
  for (int b_lo = 0; b_lo < p.nb && !rc; b_lo += slice_batches)
    rc = slice_times(b_lo, (p.nb - b_lo > slice_batches) ? b_lo + slice_batches : p.nb, b_lo == 0);
  if (rc) return rc;
  HIP_TRY(c, hipGetLastError());
  BatchTimeError bad;
  rc = read_batch_errors(c, r->d_err, &bad);
  if (rc) return rc;
  if (bad.kind) return fail_batch_time(c, bad, r->sup, /*with_event=*/false);  // (its index would be relative to a slice)
  ReconArgs a = recon_args(c, r);
  const bool one_slice = p.nb <= slice_batches;  // (its batch times are those the validation pass has just written)
  for (int b_lo = 0; b_lo < p.nb; b_lo += slice_batches) {
    const int b_hi = (p.nb - b_lo > slice_batches) ? b_lo + slice_batches : p.nb;
    if (!one_slice) {
      rc = slice_times(b_lo, b_hi, false);
      if (rc) return rc;
    }
    a.xy = src.d_xy + (int64_t)b_lo * B; a.stride = r->rate;
    a.batch_t = s.d_bt; a.nb = b_hi - b_lo;
    a.n = (int)p.packed(b_lo, b_hi);
    launch_recon_votes(a, c->stream);
  }
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  r->n_sampled += p.n_packed;
  return CMX_OK;
}

int cmx_backend_recon_add(cmx_ctx *c, int64_t n, const uint16_t *x, const uint16_t *y, const int64_t *t_ns) {
  int rc = recon_enter(c, true);
  if (rc) return rc;
  return recon_add_host(c, EventSource::arrays(n, x, y, t_ns));
}

int cmx_backend_recon_add_aos(cmx_ctx *c, int64_t n, const void *events, const cmx_aos_layout *layout) {
  int rc = recon_enter(c, true);
  if (rc) return rc;
  EventSource src;
  rc = make_aos(c, n, events, layout, &src);
  if (rc) return rc;
  return recon_add_host(c, src);
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
