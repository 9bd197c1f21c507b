// cmx_reconstruct.cpp -- cmx_backend_recon_*: the panorama of ALL events warped along the FINAL trajectory, for a spline of any knot
// count.  One call of recon_add* (cmx_recon_feed.cpp) adds the votes of exactly the events handed in into a plane that belongs to
// the reconstruction alone: no old / new split, no alpha, no IG, no blur, and nothing of the window state, the resident evaluation
// point, the map or the exchange sets is touched.  Here: the life cycle of that plane and its spline (begin, restart, extend, end),
// the whole-trajectory contrast and its gradient with respect to a left increment of EVERY control pose (recon_contrast,
// recon_grad_get, recon_eval_from): the image pass over the plane and a second pass over the same events, in the adjoint form of the
// window path -- per batch one 3-vector through the 3 x 3N spline Jacobian, so nothing grows with the knot count
// but the 2 x 3K sums -- and the plane's way out (get, render); the same for the ON / OFF planes of the signed polarity map
// (pol_get, pol_render, pol_reset) and for the planes of a set of pinhole views (view_begin, view_get, view_render,
// view_reset, view_end) and for the bins of a set of voxel grids (voxel_begin, voxel_get, voxel_get_device, voxel_reset,
// voxel_end) and for the cells of a set of time surfaces (surface_begin, surface_get, surface_get_device, surface_decay,
// surface_decay_device, surface_reset, surface_end).  Events bound once and evaluated many times, the frozen head, the
// growing binding and the native solve's hooks: cmx_recon_bound.cpp.
// Kernels: cmx_recon.hip.
#include "cmx_recon_state.hpp"

// Raw events per internal slice (a whole number of batches).  Staging -- two slots of pinned + device memory for the packed events
// and the batch times -- is bounded by this, not by the length of the input; at 2048 packed events per workgroup a full slice is
// 2048 workgroups, eight per compute unit.
constexpr int64_t kSliceEvents = 1 << 22;
static std::atomic<int64_t> g_slice_events{kSliceEvents};
int recon_diag_slice_events(int n) {  // CMX_DIAG_RECON_SLICE_EVENTS: small inputs through the multi-slice path (tests)
  if (n < 0 || n > kMaxSliceEvents) return CMX_ERR_INVALID_ARG;
  g_slice_events.store(n > 0 ? (int64_t)n : kSliceEvents, std::memory_order_relaxed);
  return CMX_OK;
}

hipError_t recon_wait(cmx_ctx *c, ReconState *r) {
  r->host_waits++;
  return hipStreamSynchronize(c->stream);
}
void frozen_drop(cmx_ctx *c, ReconState *r) {
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
  if (r->copy_stream) (void)hipStreamSynchronize(r->copy_stream);
  if (r->down_stream) (void)hipStreamSynchronize(r->down_stream);
  r->release();
  delete r;
  c->recon = nullptr;
}

int recon_enter(cmx_ctx *c, bool need_begun) {
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
int recon_start_over(cmx_ctx *c, ReconState *r, const double *knots_xyzw, bool from_base, bool staged) {
  const size_t np = (size_t)c->Wp * c->Hp;
  const ReconFrozen &fz = r->frozen;
  const bool base = from_base && fz.num_fixed > 0;
  r->grad_open = false;
  r->score_open = false;
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

int recon_slice_batches(const ReconState *r) { return slice_batches_of(g_slice_events.load(std::memory_order_relaxed), r->B); }
int recon_plan(cmx_ctx *c, const ReconState *r, int64_t n, BatchPlan *p, int *slice_batches) {
  if (!plan_batches(n, r->B, r->rate, p)) return fail(c, CMX_ERR_INVALID_ARG, "too many batches");
  *slice_batches = recon_slice_batches(r);
  return CMX_OK;
}

ReconArgs recon_args(const cmx_ctx *c, const ReconState *r) {
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

ReconGatherArgs recon_gather_args(const cmx_ctx *c, const ReconState *r) {
  ReconGatherArgs g{};
  g.ev = recon_args(c, r);
  g.itilde = r->d_jt;
  g.cx = r->d_cx; g.cy = r->d_cy; g.r = r->radius;
  g.gsum = r->d_gsum;
  g.n_voted = r->d_voted;
  return g;
}

int recon_pass_enter(cmx_ctx *c, ReconState *r, bool grad) {
  if (!grad) { r->grad_open = false; r->score_open = false; return CMX_OK; }  // (votes follow: Jt and S no longer belong to the plane)
  if (!r->grad_open) return fail(c, CMX_ERR_STATE, "no gradient pass is open (cmx_backend_recon_contrast with want_grad, and no add since)");
  return CMX_OK;
}

int recon_refuse_released(cmx_ctx *c, const ReconState *r, const char *what) {
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
  rc = recon_pol_clear(c, c->recon);  // (... nor what the polarity planes hold)
  if (rc) return rc;
  ReconState *r = c->recon;
  for (ReconTargetSet *t : {&r->views, &r->voxels, &r->surfaces}) {  // (... nor the sets' planes and cells; the targets themselves stay)
    rc = recon_set_clear(c, t);
    if (rc) return rc;
  }
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
int recon_grad_precheck(cmx_ctx *c, ReconState *r, double sigma) {
  const int rc = recon_setup_blur(c, r, sigma);
  if (rc) return rc;
  if (!(c->Wp > 2 * r->radius + 1 && c->Hp > 2 * r->radius + 1))
    return fail(c, CMX_ERR_INVALID_ARG, "panorama %d x %d too small for the adjoint gradient at blur radius %d", c->Wp, c->Hp, r->radius);
  return CMX_OK;
}

// the plane as an image pass reads it (its fp32 view refreshed), its tiles and their occupancy flags, queued
static int recon_image_source(cmx_ctx *c, ReconState *r, ImgArgs &a) {
  a.W = c->Wp; a.H = c->Hp;
  a.src_a = r->d_plane;
  a.P = 0;
  a.tiles_x = (a.W + kTileX - 1) / kTileX;
  a.tiles_y = (a.H + kTileY - 1) / kTileY;
  a.nblk = a.tiles_x * a.tiles_y;
  if (!r->d_tflags) HIP_TRY(c, hipMalloc((void **)&r->d_tflags, (size_t)a.nblk));
  recon_refresh_plane(c, r);
  HIP_TRY(c, hipMemsetAsync(r->d_tflags, 0, (size_t)a.nblk, c->stream));
  launch_tile_flags(r->d_plane, a.W, a.H, r->d_tflags, c->stream);
  a.flags_cur = r->d_tflags;
  return CMX_OK;
}

// The image pass over the plane as accumulated so far: contrast of GaussianBlur(plane, sigma), and with want_grad
// Jt = G^T (G plane) for the gradient pass it opens.  The plane is read only.
// Everything of it up to the wait: queued on the stream, contrast and mean on their way into cm[2] (host memory that stays valid
// until the caller has waited for the stream); with want_grad the gradient pass is open from here on, and r->mu is the caller's to
// set from cm[1] after its wait.
int recon_contrast_queue(cmx_ctx *c, ReconState *r, double blur_sigma, int contrast_measure, int want_grad, double *cm) {
  if (!std::isfinite(blur_sigma)) return fail(c, CMX_ERR_INVALID_ARG, "blur_sigma is not finite");
  int rc = want_grad ? recon_grad_precheck(c, r, blur_sigma) : recon_setup_blur(c, r, blur_sigma);
  if (rc) return rc;
  const int rad = r->radius;
  const size_t np = (size_t)c->Wp * c->Hp;
  ImgAdjArgs ia{};
  ImgArgs &a = ia.img;
  a.r = rad;
  memcpy(a.taps, r->taps, sizeof(a.taps));
  a.nblk = ((c->Wp + kTileX - 1) / kTileX) * ((c->Hp + kTileY - 1) / kTileY);
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
  rc = recon_image_source(c, r, a);
  if (rc) return rc;
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
  if (!rc) rc = recon_add_source(c, src, false);
  if (!rc) rc = cmx_backend_recon_contrast(c, blur_sigma, contrast_measure, grad != nullptr, contrast);
  if (!rc && grad) rc = recon_add_source(c, src, true);
  if (!rc && grad) rc = cmx_backend_recon_grad_get(c, grad);
  return rc;
}


// the plane as fp32 on the device: in deterministic mode the current fixed-point sums, converted (they stay: votes may follow)
static void recon_refresh_plane(cmx_ctx *c, ReconState *r) {
  if (r->deterministic) launch_recon_fixed_to_float(r->d_fixed, r->d_plane, (size_t)c->Wp * c->Hp, c->stream);
}

// ---- per-event support scores: the pass that cmx_backend_recon_score* (cmx_recon_feed.cpp) reads.  score_open forms S = G plane from
// the plane as it stands -- the fp32 view of the fixed-point plane in deterministic mode -- and the pass stays open until votes or
// knots change (recon_pass_enter, recon_start_over).  sigma 0: S is the plane itself, which nothing writes while the pass is open.
int cmx_backend_recon_score_open(cmx_ctx *c, double blur_sigma) {
  int rc = recon_enter(c, true);
  if (rc) return rc;
  ReconState *r = c->recon;
  if (!std::isfinite(blur_sigma)) return fail(c, CMX_ERR_INVALID_ARG, "blur_sigma is not finite");
  rc = recon_setup_blur(c, r, blur_sigma);  // (as recon_contrast: an open gradient pass at another sigma is closed, one at this sigma stays)
  if (rc) return rc;
  const int rad = r->radius;
  if (!(c->Wp > 2 * rad + 1 && c->Hp > 2 * rad + 1))  // (the own contribution of an event folds single reflections, as the adjoint gradient does)
    return fail(c, CMX_ERR_INVALID_ARG, "panorama %d x %d too small for support scores at blur radius %d", c->Wp, c->Hp, rad);
  const size_t np = (size_t)c->Wp * c->Hp;
  r->score_open = false;  // (a call refused above leaves an open pass as it was: it has its own taps)
  if (rad > 0) {
    if (!r->d_support) HIP_TRY(c, hipMalloc((void **)&r->d_support, np * sizeof(float)));
    ImgArgs a{};
    a.r = rad;
    memcpy(a.taps, r->taps, sizeof(a.taps));
    rc = recon_image_source(c, r, a);
    if (rc) return rc;
    // S is read wherever ANY event lands, not only where votes lie: zero first, then the tiles with a vote within reach
    HIP_TRY(c, hipMemsetAsync(r->d_support, 0, np * sizeof(float), c->stream));
    launch_recon_smooth(a, r->d_support, c->stream);
  } else {
    recon_refresh_plane(c, r);
  }
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, recon_wait(c, r));
  r->score_radius = rad;
  memcpy(r->score_taps, r->taps, sizeof(r->score_taps));
  r->score_open = true;
  return CMX_OK;
}

int recon_score_enter(cmx_ctx *c) {
  const int rc = recon_enter(c, true);
  if (rc) return rc;
  if (!c->recon->score_open)
    return fail(c, CMX_ERR_STATE, "no score pass is open (cmx_backend_recon_score_open, and nothing that changes the plane or the knots since)");
  return CMX_OK;
}

int cmx_backend_recon_score_plane(cmx_ctx *c, float *S) {
  int rc = recon_score_enter(c);
  if (rc) return rc;
  if (!S) return fail(c, CMX_ERR_INVALID_ARG, "null output");
  ReconState *r = c->recon;
  const float *src = r->score_radius > 0 ? r->d_support : r->d_plane;
  HIP_TRY(c, hipMemcpyAsync(S, src, (size_t)c->Wp * c->Hp * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return CMX_OK;
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

// ---- signed polarity map: the ON / OFF planes of cmx_backend_recon_pol_add* (cmx_recon_feed.cpp)
int recon_pol_clear(cmx_ctx *c, ReconState *r) {
  if (!r->d_pol) return CMX_OK;
  const size_t np2 = 2 * (size_t)c->Wp * c->Hp;
  HIP_TRY(c, hipMemsetAsync(r->d_pol, 0, np2 * sizeof(float), c->stream));
  if (r->d_pol_fixed) HIP_TRY(c, hipMemsetAsync(r->d_pol_fixed, 0, np2 * sizeof(unsigned long long), c->stream));
  HIP_TRY(c, hipMemsetAsync(r->d_pol_inside, 0, 2 * sizeof(unsigned long long), c->stream));
  return CMX_OK;
}
int recon_pol_ensure(cmx_ctx *c, ReconState *r) {
  if (r->d_pol) return CMX_OK;
  const size_t np2 = 2 * (size_t)c->Wp * c->Hp;
  float *plane = nullptr;
  unsigned long long *fixed = nullptr, *inside = nullptr;
  hipError_t e = hipMalloc((void **)&plane, np2 * sizeof(float));
  if (e == hipSuccess && r->deterministic) e = hipMalloc((void **)&fixed, np2 * sizeof(unsigned long long));
  if (e == hipSuccess) e = hipMalloc((void **)&inside, 2 * sizeof(unsigned long long));
  if (e != hipSuccess) {  // (all three or none: d_pol says whether the planes exist)
    (void)hipFree(plane); (void)hipFree(fixed); (void)hipFree(inside);
    return fail(c, CMX_ERR_HIP, "allocating the polarity planes: %s", hipGetErrorString(e));
  }
  r->d_pol = plane; r->d_pol_fixed = fixed; r->d_pol_inside = inside;
  return recon_pol_clear(c, r);
}

int cmx_backend_recon_pol_reset(cmx_ctx *c) {
  int rc = recon_enter(c, true);
  if (rc) return rc;
  rc = recon_pol_clear(c, c->recon);
  if (rc) return rc;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return CMX_OK;
}

// the two planes as fp32 on the device: in deterministic mode the current fixed-point sums, converted (they stay: votes may follow)
static void recon_pol_refresh(cmx_ctx *c, ReconState *r) {
  if (r->d_pol_fixed) launch_recon_fixed_to_float(r->d_pol_fixed, r->d_pol, 2 * (size_t)c->Wp * c->Hp, c->stream);
}

int cmx_backend_recon_pol_get(cmx_ctx *c, float *on, float *off, int64_t *n_on, int64_t *n_off) {
  int rc = recon_enter(c, true);
  if (rc) return rc;
  ReconState *r = c->recon;
  const size_t np = (size_t)c->Wp * c->Hp;
  unsigned long long inside[2] = {0, 0};
  if (!r->d_pol) {  // (no pol_add* yet: nothing has been allocated, and nothing is)
    if (on) memset(on, 0, np * sizeof(float));
    if (off) memset(off, 0, np * sizeof(float));
  } else {
    if (on || off) {
      recon_pol_refresh(c, r);
      HIP_TRY(c, hipGetLastError());
    }
    if (on) HIP_TRY(c, hipMemcpyAsync(on, r->d_pol, np * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    if (off) HIP_TRY(c, hipMemcpyAsync(off, r->d_pol + np, np * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    if (n_on || n_off) HIP_TRY(c, hipMemcpyAsync(inside, r->d_pol_inside, sizeof(inside), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
  }
  if (n_on) *n_on = (int64_t)inside[0];
  if (n_off) *n_off = (int64_t)inside[1];
  return CMX_OK;
}

// the signed map ON - OFF as an 8-bit image (cmx_display.hip): one range reduction and one tone pass over the difference of the planes
int cmx_backend_recon_pol_render(cmx_ctx *c, double gamma, int mode, unsigned char *out) {
  int rc = recon_enter(c, true);
  if (rc) return rc;
  if (!out) return fail(c, CMX_ERR_INVALID_ARG, "null output buffer");
  if (!std::isfinite(gamma) || !(gamma > 0.0)) return fail(c, CMX_ERR_INVALID_ARG, "gamma must be finite and > 0");
  if (mode != CMX_POL_MONO8 && mode != CMX_POL_BGR8) return fail(c, CMX_ERR_INVALID_ARG, "unknown render mode %d", mode);
  ReconState *r = c->recon;
  const size_t np = (size_t)c->Wp * c->Hp, bytes = mode == CMX_POL_BGR8 ? 3 * np : np;
  if (!r->d_pol) {  // (no pol_add* yet: the neutral image)
    memset(out, mode == CMX_POL_BGR8 ? 255 : 128, bytes);
    return CMX_OK;
  }
  rc = display_begin(c, bytes);
  if (rc) return rc;
  recon_pol_refresh(c, r);
  launch_display_range_signed(r->d_pol, r->d_pol + np, np, c->d_disp_range, c->stream);
  launch_display_signed(r->d_pol, r->d_pol + np, np, (float)gamma, mode == CMX_POL_BGR8, c->d_disp_range, c->d_disp, c->stream);
  return display_deliver(c, bytes, out);
}

// ---- target sets: the pinhole views, voxel grids and time surfaces that cmx_backend_recon_view_add* / _voxel_add* / _surface_add*
// (cmx_recon_feed.cpp) vote into, and their contents' way out.  One ReconTargetSet each and one copy of everything they share; a
// call names its set by member (&ReconState::views ...), since the reconstruction may not exist yet when it does.
static void recon_set_free(cmx_ctx *c, ReconState *r, ReconTargetSet *t) {
  if (!t->d_entries) return;
  (void)hipStreamSynchronize(c->stream);  // (a vote pass queued earlier may still write the planes or cells)
  t->release();
  if (t == &r->surfaces) {
    (void)hipFree(r->d_stref); (void)hipFree(r->d_sdecay);
    r->d_stref = nullptr; r->d_sdecay = nullptr; r->sdecay_cap = 0;
  }
}

int recon_set_clear(cmx_ctx *c, ReconTargetSet *t) {
  if (!t->d_entries) return CMX_OK;
  const size_t nc = (size_t)t->n * t->cells_per_target();
  if (t->timestamps) {  // every cell = "no event yet": INT64_MIN, a pattern no byte memset writes
    launch_recon_surface_fill(t->d_cells, nc, c->stream);
    HIP_TRY(c, hipGetLastError());
  } else {
    HIP_TRY(c, hipMemsetAsync(t->d_planes, 0, nc * sizeof(float), c->stream));
    if (t->d_fixed) HIP_TRY(c, hipMemsetAsync(t->d_fixed, 0, nc * sizeof(unsigned long long), c->stream));
  }
  HIP_TRY(c, hipMemsetAsync(t->d_voted, 0, (size_t)t->n * sizeof(unsigned long long), c->stream));
  return CMX_OK;
}

int recon_set_enter(cmx_ctx *c, ReconTargetSet ReconState::*which) {
  const int rc = recon_enter(c, true);
  if (rc) return rc;
  const ReconTargetSet &t = c->recon->*which;
  if (!t.d_entries) return fail(c, CMX_ERR_STATE, "cmx_backend_recon_%s_begin has not succeeded", t.api);
  return CMX_OK;
}

// the common front door of get*, render and decay*: the set, and a range of targets inside it
static int recon_set_range(cmx_ctx *c, ReconTargetSet ReconState::*which, int first, int count) {
  const int rc = recon_set_enter(c, which);
  if (rc) return rc;
  const ReconTargetSet &t = c->recon->*which;
  if (first < 0 || count < 0 || first > t.n || count > t.n - first)
    return fail(c, CMX_ERR_INVALID_ARG, "%ss [%d, %d + %d) outside the %d of the set", t.noun, first, first, count, t.n);
  return CMX_OK;
}

static int recon_set_reset(cmx_ctx *c, ReconTargetSet ReconState::*which) {
  int rc = recon_set_enter(c, which);
  if (rc) return rc;
  rc = recon_set_clear(c, &(c->recon->*which));
  if (rc) return rc;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return CMX_OK;
}

static int recon_set_end(cmx_ctx *c, ReconTargetSet ReconState::*which) {
  const int rc = recon_enter(c, true);
  if (rc) return rc;
  recon_set_free(c, c->recon, &(c->recon->*which));  // (no set: nothing to free, not an error)
  return CMX_OK;
}

// the argument rules of ONE target and its entry as the kernels read it: R(quat)^T from the normalised quaternion
static int recon_view_entry(cmx_ctx *c, const cmx_recon_view &v, int i, ReconViewDev *out) {
  const double *q = v.quat_xyzw;
  const double nrm = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  if (!std::isfinite(nrm) || !(nrm > 0.0)) return fail(c, CMX_ERR_INVALID_ARG, "view %d: the quaternion has no direction", i);
  if (!std::isfinite(v.fx) || !std::isfinite(v.fy) || !(v.fx > 0.0) || !(v.fy > 0.0))
    return fail(c, CMX_ERR_INVALID_ARG, "view %d: fx, fy must be finite and > 0", i);
  if (!std::isfinite(v.cx) || !std::isfinite(v.cy)) return fail(c, CMX_ERR_INVALID_ARG, "view %d: cx, cy must be finite", i);
  if (v.t_lo_ns >= v.t_hi_ns) return fail(c, CMX_ERR_INVALID_ARG, "view %d: empty time range", i);
  const Mat3 R = q_to_R(Quat{q[0] / nrm, q[1] / nrm, q[2] / nrm, q[3] / nrm});
  ReconViewDev &d = *out;
  for (int a = 0; a < 3; a++)
    for (int b = 0; b < 3; b++) d.Rt[3 * a + b] = R.m[3 * b + a];
  d.fx = v.fx; d.fy = v.fy; d.cx = v.cx; d.cy = v.cy;
  d.t_lo = (long long)v.t_lo_ns; d.t_hi = (long long)v.t_hi_ns;
  d.index = i;
  return CMX_OK;
}

// What a _begin call asks for.  Entry: the set's entry type, a ReconViewDev or a struct that starts with one.  limits: the set's own
// rules on n and per, checked after the size and before the cell count; extra: its own rule on target i and whatever its entry adds,
// after recon_view_entry.  `what` names the request in the two messages that speak of all of it.
template <typename Entry, typename Limits, typename Extra>
static int recon_set_begin(cmx_ctx *c, ReconTargetSet ReconState::*which, int W, int H, int n, int per, bool polarity, const cmx_recon_view *targets,
                           const char *what, Limits limits, Extra extra) {
  int rc = recon_enter(c, true);
  if (rc) return rc;
  ReconState *r = c->recon;
  ReconTargetSet *t = &(r->*which);
  if (W < 4 || W > 8192 || H < 4 || H > 8192) return fail(c, CMX_ERR_INVALID_ARG, "%s size %d x %d outside [4, 8192]", t->noun, W, H);
  rc = limits();
  if (rc) return rc;
  if ((long long)n * per * W * H > (1LL << 28)) return fail(c, CMX_ERR_INVALID_ARG, "%s: more than 2^28 cells", what);
  if (!targets) return fail(c, CMX_ERR_INVALID_ARG, "null %s array", t->noun);
  std::vector<Entry> dev((size_t)n);
  std::vector<ReconViewRange> ranges((size_t)n);
  for (int i = 0; i < n; i++) {
    ReconViewDev *v = reinterpret_cast<ReconViewDev *>(&dev[(size_t)i]);
    rc = recon_view_entry(c, targets[i], i, v);
    if (!rc) rc = extra(i, targets[i], &dev[(size_t)i]);
    if (rc) return rc;
    ranges[(size_t)i] = ReconViewRange{v->t_lo, v->t_hi};
  }
  recon_set_free(c, r, t);  // a second begin starts over
  ReconTargetSet s{t->noun, t->api, t->timestamps};
  const size_t nc = (size_t)n * per * W * H;
  hipError_t e = hipMalloc(&s.d_entries, dev.size() * sizeof(Entry));
  if (e == hipSuccess) e = hipMalloc((void **)&s.d_ranges, ranges.size() * sizeof(ReconViewRange));
  if (e == hipSuccess && s.timestamps) e = hipMalloc((void **)&s.d_cells, nc * sizeof(long long));
  if (e == hipSuccess && !s.timestamps) e = hipMalloc((void **)&s.d_planes, nc * sizeof(float));
  if (e == hipSuccess && !s.timestamps && r->deterministic) e = hipMalloc((void **)&s.d_fixed, nc * sizeof(unsigned long long));
  if (e == hipSuccess) e = hipMalloc((void **)&s.d_voted, (size_t)n * sizeof(unsigned long long));
  if (e == hipSuccess && t == &r->surfaces) e = hipMalloc((void **)&r->d_stref, (size_t)n * sizeof(long long));
  if (e == hipSuccess) e = hipMemcpy(s.d_entries, dev.data(), dev.size() * sizeof(Entry), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(s.d_ranges, ranges.data(), ranges.size() * sizeof(ReconViewRange), hipMemcpyHostToDevice);
  if (e != hipSuccess) {  // (all of it or none: d_entries says whether the set exists)
    s.release();
    if (t == &r->surfaces) { (void)hipFree(r->d_stref); r->d_stref = nullptr; }
    return fail(c, CMX_ERR_HIP, "allocating %s: %s", what, hipGetErrorString(e));
  }
  s.n = n; s.W = W; s.H = H; s.per = per; s.polarity = polarity;
  *t = s;
  rc = recon_set_clear(c, t);
  if (rc) return rc;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return CMX_OK;
}

// targets [first, first + count) wherever `out` is (host: get; the context's device: get_device) and their counters: the timestamps as
// they are, or the vote sums as fp32 -- in deterministic mode the current fixed-point sums, converted first (they stay: votes may follow)
typedef void (*ReconFixedToFloat)(const unsigned long long *fixed, float *plane, size_t n, hipStream_t s);
static void recon_set_refresh(cmx_ctx *c, ReconTargetSet &t, int first, int count, ReconFixedToFloat convert) {
  const size_t per = t.cells_per_target();
  if (t.d_fixed) convert(t.d_fixed + (size_t)first * per, t.d_planes + (size_t)first * per, (size_t)count * per, c->stream);
}
static int recon_set_deliver(cmx_ctx *c, ReconTargetSet ReconState::*which, int first, int count, void *out, ReconFixedToFloat convert,
                             hipMemcpyKind kind, int64_t *n_voted) {
  const int rc = recon_set_range(c, which, first, count);
  if (rc || count == 0) return rc;
  ReconTargetSet &t = c->recon->*which;
  const size_t per = t.cells_per_target();
  static_assert(sizeof(int64_t) == sizeof(unsigned long long), "the counters travel as they are");
  if (out && t.timestamps) HIP_TRY(c, hipMemcpyAsync(out, t.d_cells + (size_t)first * per, (size_t)count * per * sizeof(int64_t), kind, c->stream));
  if (out && !t.timestamps) {
    recon_set_refresh(c, t, first, count, convert);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(out, t.d_planes + (size_t)first * per, (size_t)count * per * sizeof(float), kind, c->stream));
  }
  if (n_voted) HIP_TRY(c, hipMemcpyAsync(n_voted, t.d_voted + first, (size_t)count * sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return CMX_OK;
}
// ... into memory of the context's device
static int recon_set_deliver_device(cmx_ctx *c, ReconTargetSet ReconState::*which, int first, int count, void *d_out, ReconFixedToFloat convert) {
  const int rc = recon_set_enter(c, which);
  if (rc) return rc;
  if (count > 0 && !d_out) return fail(c, CMX_ERR_INVALID_ARG, "null device output");
  return recon_set_deliver(c, which, first, count, d_out, convert, hipMemcpyDeviceToDevice, nullptr);
}

// ---- pinhole views
int cmx_backend_recon_view_begin(cmx_ctx *c, int Wv, int Hv, int n_views, const cmx_recon_view *views) {
  char what[96];
  snprintf(what, sizeof(what), "%d views of %d x %d", n_views, Wv, Hv);
  return recon_set_begin<ReconViewDev>(
      c, &ReconState::views, Wv, Hv, n_views, 1, false, views, what,
      [&] { return n_views < 1 || n_views > 4096 ? fail(c, CMX_ERR_INVALID_ARG, "n_views=%d outside [1, 4096]", n_views) : (int)CMX_OK; },
      [](int, const cmx_recon_view &, ReconViewDev *) { return (int)CMX_OK; });
}
int cmx_backend_recon_view_reset(cmx_ctx *c) { return recon_set_reset(c, &ReconState::views); }
int cmx_backend_recon_view_end(cmx_ctx *c) { return recon_set_end(c, &ReconState::views); }
int cmx_backend_recon_view_get(cmx_ctx *c, int first_view, int count, float *planes, int64_t *n_voted) {
  return recon_set_deliver(c, &ReconState::views, first_view, count, planes, launch_recon_fixed_to_float, hipMemcpyDeviceToHost, n_voted);
}

// cmx_backend_recon_render's tone map, without the outline, on one view's plane
int cmx_backend_recon_view_render(cmx_ctx *c, int view, double gamma, unsigned char *out) {
  int rc = recon_set_enter(c, &ReconState::views);
  if (rc) return rc;
  ReconTargetSet &t = c->recon->views;
  if (view < 0 || view >= t.n) return fail(c, CMX_ERR_INVALID_ARG, "view %d outside the %d of the set", view, t.n);
  if (!out) return fail(c, CMX_ERR_INVALID_ARG, "null output buffer");
  if (!std::isfinite(gamma) || !(gamma > 0.0)) return fail(c, CMX_ERR_INVALID_ARG, "gamma must be finite and > 0");
  const size_t np = t.cells_per_target();
  rc = display_begin(c, np);
  if (rc) return rc;
  recon_set_refresh(c, t, view, 1, launch_recon_fixed_to_float);
  const float *plane = t.d_planes + (size_t)view * np;
  launch_display_range(plane, nullptr, np, c->d_disp_range, c->stream);
  launch_display_map(plane, np, (float)gamma, false, c->d_disp_range, c->d_disp, c->stream);
  return display_deliver(c, np, out);
}

// ---- voxel grids: a grid is a view with a bin axis over its time range; the planes are grid-major, n_bins to a grid, and their
// fixed-point twins hold signed sums
int cmx_backend_recon_voxel_begin(cmx_ctx *c, int Wv, int Hv, int n_bins, int signed_polarity, int n_grids, const cmx_recon_view *grids) {
  char what[96];
  snprintf(what, sizeof(what), "%d grids of %d bins of %d x %d", n_grids, n_bins, Wv, Hv);
  return recon_set_begin<ReconVoxelDev>(
      c, &ReconState::voxels, Wv, Hv, n_grids, n_bins, signed_polarity != 0, grids, what,
      [&] {
        if (n_bins < 1 || n_bins > 64) return fail(c, CMX_ERR_INVALID_ARG, "n_bins=%d outside [1, 64]", n_bins);
        if (n_grids < 1 || (long long)n_grids * n_bins > 4096)
          return fail(c, CMX_ERR_INVALID_ARG, "%d grids of %d bins: n_grids * n_bins outside [1, 4096]", n_grids, n_bins);
        return (int)CMX_OK;
      },
      [&](int i, const cmx_recon_view &g, ReconVoxelDev *d) {
        // t_lo < t_hi: their difference as an unsigned number is exact, whatever the two are -- no signed overflow.  The bin axis needs
        // a finite span: beyond 2^53 ns the fp64 image of (t - t_lo) is no longer exact, so "all time" is refused
        const uint64_t span = (uint64_t)g.t_hi_ns - (uint64_t)g.t_lo_ns;
        if (span > (1ull << 53)) return fail(c, CMX_ERR_INVALID_ARG, "grid %d: time range longer than 2^53 ns (the bin axis needs a finite span)", i);
        d->scale = (double)(n_bins - 1) / (double)span;
        return (int)CMX_OK;
      });
}
int cmx_backend_recon_voxel_reset(cmx_ctx *c) { return recon_set_reset(c, &ReconState::voxels); }
int cmx_backend_recon_voxel_end(cmx_ctx *c) { return recon_set_end(c, &ReconState::voxels); }
int cmx_backend_recon_voxel_get(cmx_ctx *c, int first_grid, int count, float *out, int64_t *n_voted) {
  return recon_set_deliver(c, &ReconState::voxels, first_grid, count, out, launch_recon_fixed_to_float_signed, hipMemcpyDeviceToHost, n_voted);
}
int cmx_backend_recon_voxel_get_device(cmx_ctx *c, int first_grid, int count, float *d_out) {
  return recon_set_deliver_device(c, &ReconState::voxels, first_grid, count, d_out, launch_recon_fixed_to_float_signed);
}

// ---- time surfaces: a surface is a view; the cells are surface-major, C = 1 or 2 channels to a surface, ON before OFF, and leave as
// they are (get, get_device: absolute nanoseconds, INT64_MIN where no event landed) or through an exponential decay (decay, decay_device)
int cmx_backend_recon_surface_begin(cmx_ctx *c, int Wv, int Hv, int by_polarity, int n_surfaces, const cmx_recon_view *surfaces) {
  const int C = by_polarity ? 2 : 1;
  char what[96];
  snprintf(what, sizeof(what), "%d surfaces of %d channels of %d x %d", n_surfaces, C, Wv, Hv);
  return recon_set_begin<ReconViewDev>(
      c, &ReconState::surfaces, Wv, Hv, n_surfaces, C, by_polarity != 0, surfaces, what,
      [&] { return n_surfaces < 1 || n_surfaces > 4096 ? fail(c, CMX_ERR_INVALID_ARG, "n_surfaces=%d outside [1, 4096]", n_surfaces) : (int)CMX_OK; },
      [&](int i, const cmx_recon_view &s, ReconViewDev *) {
        // INT64_MIN marks a cell no event has reached; a range that starts there could hold an event with that timestamp
        if (s.t_lo_ns == INT64_MIN) return fail(c, CMX_ERR_INVALID_ARG, "surface %d: t_lo_ns is INT64_MIN, the empty marker", i);
        return (int)CMX_OK;
      });
}
int cmx_backend_recon_surface_reset(cmx_ctx *c) { return recon_set_reset(c, &ReconState::surfaces); }
int cmx_backend_recon_surface_end(cmx_ctx *c) { return recon_set_end(c, &ReconState::surfaces); }
int cmx_backend_recon_surface_get(cmx_ctx *c, int first, int count, int64_t *cells, int64_t *n_voted) {
  return recon_set_deliver(c, &ReconState::surfaces, first, count, cells, nullptr, hipMemcpyDeviceToHost, n_voted);
}
int cmx_backend_recon_surface_get_device(cmx_ctx *c, int first, int count, int64_t *d_cells) {
  return recon_set_deliver_device(c, &ReconState::surfaces, first, count, d_cells, nullptr);
}

// one decay pass over surfaces [first, first + count) into d_out on the device, queued; t_ref_ns (host, count values) or NULL: every
// surface's own t_hi
static int recon_surface_decay_queue(cmx_ctx *c, int first, int count, const int64_t *t_ref_ns, double tau_ns, float *d_out) {
  ReconState *r = c->recon;
  const ReconTargetSet &t = r->surfaces;
  const long long *d_tref = nullptr;
  if (t_ref_ns) {  // (pageable memory: the copy has read it when the call returns)
    HIP_TRY(c, hipMemcpyAsync(r->d_stref, t_ref_ns, (size_t)count * sizeof(int64_t), hipMemcpyHostToDevice, c->stream));
    d_tref = r->d_stref;
  }
  launch_recon_surface_decay(t.d_cells + (size_t)first * t.cells_per_target(), t.d_ranges + first, d_tref, t.cells_per_target(), count, tau_ns,
                             d_out, c->stream);
  HIP_TRY(c, hipGetLastError());
  return CMX_OK;
}
static int recon_surface_decay_checks(cmx_ctx *c, int first, int count, double tau_ns, const void *out) {
  const int rc = recon_set_range(c, &ReconState::surfaces, first, count);
  if (rc) return rc;
  if (!std::isfinite(tau_ns) || !(tau_ns > 0.0)) return fail(c, CMX_ERR_INVALID_ARG, "tau_ns must be finite and > 0");
  if (count > 0 && !out) return fail(c, CMX_ERR_INVALID_ARG, "null output");
  return CMX_OK;
}
int cmx_backend_recon_surface_decay_device(cmx_ctx *c, int first, int count, const int64_t *t_ref_ns, double tau_ns, float *d_out) {
  int rc = recon_surface_decay_checks(c, first, count, tau_ns, d_out);
  if (rc || count == 0) return rc;
  rc = recon_surface_decay_queue(c, first, count, t_ref_ns, tau_ns, d_out);
  if (rc) return rc;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return CMX_OK;
}
int cmx_backend_recon_surface_decay(cmx_ctx *c, int first, int count, const int64_t *t_ref_ns, double tau_ns, float *out) {
  int rc = recon_surface_decay_checks(c, first, count, tau_ns, out);
  if (rc || count == 0) return rc;
  ReconState *r = c->recon;
  const size_t n = (size_t)count * r->surfaces.cells_per_target();
  rc = ensure(c, r->d_sdecay, r->sdecay_cap, n);  // (the decayed cells exist nowhere else: the set holds timestamps)
  if (rc) return rc;
  rc = recon_surface_decay_queue(c, first, count, t_ref_ns, tau_ns, r->d_sdecay);
  if (rc) return rc;
  HIP_TRY(c, hipMemcpyAsync(out, r->d_sdecay, n * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return CMX_OK;
}
