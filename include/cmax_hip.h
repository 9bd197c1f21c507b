/*
 * cmax_hip.h -- C ABI of libcmaxhip.so: MI355X (gfx950) evaluator for cmax_slam's event-warping hot path.
 *
 * This is the drop-in boundary.  The reference sits behind GSL's
 *   gsl_multimin_function_fdf { f, df, fdf, n, params }
 * filled at src/frontend/local_optim_contrast_gsl.cpp:87-96 and src/backend/global_optim_contrast_gsl.cpp:23-33.
 * The bodies of local_contrast_{f,df,fdf} / global_contrast_{f,df,fdf} become ~10-line calls into the entry
 * points below (INTEGRATION.md shows them); everything they used to compute on the CPU
 *   (computeImageOfWarpedEvents + computeContrast) runs as hand-written HIP kernels.
 *
 * Conventions
 *   - plain C types only; every entry point returns an int status (CMX_OK == 0) and never aborts the host
 *     (the reference's glog CHECK / Basalt assert / std::out_of_range abort paths become error codes).
 *   - a context owns all device memory; inputs are copied at set_*; outputs go to caller buffers.
 *   - one context per path (front end / back end); contexts are independent and may be driven from two
 *     host threads concurrently (src/node.cpp:22 + src/cmax_slam.cpp:92); one context is not thread-safe.
 *   - eval() is synchronous: it returns when contrast / gradient are on the host.
 *   - contrast and gradient are returned with the reference's sign (maximised quantity); the GSL glue
 *     negates them exactly as local_optim_contrast_gsl.cpp:48-55 does.
 *   - quaternions are (x, y, z, w) (Eigen coeffs() order); matrices row-major.
 */
#ifndef CMAX_HIP_H
#define CMAX_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
#if defined(__GNUC__)
#pragma GCC visibility push(default) /* the library is built with -fvisibility=hidden: exactly these symbols are exported */
#endif

typedef struct cmx_ctx cmx_ctx;

enum {
  CMX_OK = 0,
  CMX_ERR_INVALID_ARG = 1,  /* null pointer, bad size, unsupported spline order, ... */
  CMX_ERR_EVENT_RANGE = 2,  /* an event has x >= W or y >= H (reference: std::out_of_range from .at()) */
  CMX_ERR_HIP = 3,          /* a HIP runtime call failed; see cmx_last_error() */
  CMX_ERR_SPLINE_RANGE = 4, /* a batch time lies outside the knot support (reference: BASALT_ASSERT abort) */
  CMX_ERR_STATE = 5,        /* eval before set_packet / set_window, wrong context kind, ... */
  CMX_ERR_TIME_ORDER = 6    /* a batch spans a negative time interval (reference: CHECK_GE abort) */
};

/* contrast_measure: include/frontend/local_focus_funcs.h:7-11.  As in the reference's switch statements any other
 * value means VARIANCE, and the back end (global_focus_funcs.cpp:61-69) treats GRADIENT_MAGNITUDE as VARIANCE too.
 * GRADIENT_MAGNITUDE (Sobel, front end) follows CMX_OPT_GRAD_MODE like the other two: with CMX_GRAD_ADJOINT the gradient is
 * (2/N) <dW_k, G^T (Sx^T gx + Sy^T gy)>, gx / gy = Sobel of the blurred image (same results within fp32 rounding).  The
 * device-driven solve and the one-launch forms are not available for it: cmx_frontend_solve runs host-driven. */
enum { CMX_VARIANCE = 0, CMX_MEAN_SQUARE = 1, CMX_GRADIENT_MAGNITUDE = 2 };

/* how the analytic gradient is formed */
enum {
  CMX_GRAD_PLANES = 0, /* faithful: scatter P derivative planes, blur them, reduce (reference data flow) */
  CMX_GRAD_ADJOINT = 1 /* equivalent: blur is linear => grad_k = sum_events <dW_k, G^T 2(G I - mu)/N>; one extra
                          pass over the events gathers from one plane; no derivative planes */
};

/* cmx_set_option keys a HOST may need: CMX_OPT_DETERMINISTIC (bitwise reproducibility), CMX_OPT_SPIN_WAIT (how its threads wait) and
 * CMX_OPT_GRAD_MODE / CMX_OPT_SPLAT_MODE together to select the reference-shaped data flow.  That is the supported surface.  The A/B
 * switches that tests and same-box measurements use to reach every internal form on any input (forms the library otherwise selects BY
 * ITSELF from the configuration, defaulting to the fastest) live in include/cmax_hip_diag.h: same cmx_set_option, no stability promise. */
enum {
  CMX_OPT_GRAD_MODE = 1,  /* CMX_GRAD_ADJOINT (default) | CMX_GRAD_PLANES */
  CMX_OPT_SPLAT_MODE = 2, /* 0 = one global fp32 atomic per vote;
                             1 (default) = LDS-privatised: events are sorted once per packet/window by the 32x32 destination
                                 tile of their vote, workgroups accumulate in LDS and flush touched pixels; votes that
                                 leave a window (parameters drifted) take the global path, so results stay exact;
                                 applies to the plane-0 splat (cost-only evaluations and CMX_GRAD_ADJOINT) */
  CMX_OPT_DETERMINISTIC = 5, /* 1: bitwise run-to-run reproducible results (default 0).  With the LDS-privatised splat
                             (CMX_OPT_SPLAT_MODE 1, adjoint gradient or cost-only) every vote that reaches global memory
                             becomes a 64-bit integer add into a 2^-30 fixed-point plane -- integer adds commute -- and
                             one extra pass converts it to the fp32 plane; the front-end gather then walks the events in
                             time order and large panoramas do not use the compacted tile list, so that every
                             floating-point sum has a fixed order.  Costs ~10-20 % per evaluation.  The reference-shaped
                             flow (derivative planes, fp32 atomics) stays order-dependent */
  CMX_OPT_SPIN_WAIT = 4   /* ONE policy for the three places a host thread of this library waits:
                             (a) an evaluation waiting for its last kernel -- spins on a completion ticket that kernel writes to
                                 mapped host memory after the results (a few microseconds sooner than hipStreamSynchronize returns);
                             (b) a group's worker threads between two commands;  (c) a CMX_SCHED_BACKGROUND context held behind an
                                 urgent burst (cmx_set_sched_class).
                             1 (default): (a) spins for as long as the evaluation runs (the calling thread is blocked in a
                                 synchronous call either way: one core busy for its ~40-250 us); (b), (c) -- threads with NOTHING
                                 on the device -- spin for 50 us, then sleep on a condition variable: an idle group and a held back
                                 end use no core.
                             0: never spin: (a) is plain hipStreamSynchronize, (b) / (c) sleep at once.
                             n >= 2: spin budget in microseconds for all three ((a): then hipStreamSynchronize). */
};

const char *cmx_version(void);
int cmx_device_count(void);
const char *cmx_last_error(const cmx_ctx *ctx);
const char *cmx_status_string(int status);
void cmx_destroy(cmx_ctx *ctx);
int cmx_set_option(cmx_ctx *ctx, int key, int value);
/* run the context's work on a caller-owned hipStream_t (e.g. torch's current stream); NULL = own stream */
int cmx_set_stream(cmx_ctx *ctx, void *hip_stream);
/* Two paths on one GPU.  The reference runs the front end (a packet every 10 ms, src/node.cpp:22) beside the back-end thread's
 * window solves (src/cmax_slam.cpp:92); on one GPU the two contexts' kernels share the compute units.  (Stream priorities and CU masks
 * were measured not to deliver the asked-for pair of slow-downs, profiles/r04_fe_beside_be.txt: the two entry points live in
 * cmax_hip_diag.h since ABI 6.) */
/* What DOES give the front end its latency back without a static split: cooperative scheduling between the contexts of one
 * process that share a device, at evaluation granularity.  A context of class CMX_SCHED_BACKGROUND (the back end) holds its
 * NEXT evaluation -- between two evaluations of a solve there is nothing of it on the GPU -- while a context of class
 * CMX_SCHED_URGENT on the same device (the front end: a 0.5 ms solve every 10 ms) has a call of cmx_*_eval / _eval_each /
 * _solve in progress, or finished one less than 20 us ago (so that a GSL-driven sequence of evaluations counts as one burst).
 * The urgent call then waits for at most the one background evaluation already on the device.  A background context never
 * waits longer than 5 ms in a row.  Host-side only: no kernel, stream or result changes.  Default: CMX_SCHED_NORMAL (neither
 * waits nor is waited for).  Measured: bench.py frontend_beside_backend.cooperative. */
enum { CMX_SCHED_BACKGROUND = -1, CMX_SCHED_NORMAL = 0, CMX_SCHED_URGENT = 1 };
int cmx_set_sched_class(cmx_ctx *ctx, int sched_class);

/* ------------------------------------------------------------------ front end -------------------------
 * replaces AngVelEstimator::computeImageOfWarpedEvents + computeContrast
 *   (src/frontend/local_image_warped_events.cpp:10-170, src/frontend/local_focus_funcs.cpp:82-120)
 * as called from local_contrast_fdf (src/frontend/local_optim_contrast_gsl.cpp:20-56). */

/* lut: W*H*3 fp64 bearing vectors, index (y*W+x)*3 -- the reference's precomputed_bearing_vectors
 * (src/cmax_slam.cpp:106-120); copied to the device once. */
int cmx_frontend_create(cmx_ctx **out, int device, int W, int H, const double *lut);

/* ------------------------------------------------------------------ events as the host holds them (AoS) ------
 * The reference keeps its events as std::vector<dvs_msgs::Event> (src/frontend/ang_vel_estimator.cpp:68-147: pushEvent / the
 * per-packet copy into event_subset_; src/backend/pose_graph_optimizer.cpp:131-165: getEventSubset) -- an array of
 *   struct { uint16_t x, y; struct { uint32_t sec, nsec; } ts; uint8_t polarity; }        (16 bytes)
 * The *_aos entry points take that memory as it is: ONE packing pass on the host pool straight from the array into the pinned
 * upload buffer (x | y << 16 [| old << 31]; t_ns = sec * 1e9 + nsec formed on the fly for the batch times / the store's
 * timestamps), no intermediate x[] / y[] / t_ns[] vectors.  `layout` describes any array of records: record size and the byte
 * offsets of the four fields (uint16 x, uint16 y, uint32 sec, uint32 nsec); CMX_AOS_DVS_EVENT is dvs_msgs::Event's.  Same
 * checks, same errors, bit-identical device contents as the SoA entry points given the same events. */
typedef struct { size_t stride, off_x, off_y, off_sec, off_nsec; } cmx_aos_layout;
#define CMX_AOS_DVS_EVENT {16, 0, 2, 4, 8}
/* The calls that read polarity (cmx_events_push_aos_pol, cmx_backend_recon_pol_add_aos) take the byte offset of a one-byte
 * polarity field inside the record beside the layout (nonzero = ON); CMX_AOS_DVS_POLARITY is dvs_msgs::Event's.  The layout
 * struct itself stays as it is: it is passed by pointer and its size is part of the ABI. */
#define CMX_AOS_DVS_POLARITY 12

/* State AngVelEstimator hands over before a solve (src/frontend/ang_vel_estimator.cpp:137-147):
 * event_subset_ (SoA here; polarity is never read), time_packet_, camera_matrix_ (fx,fy,cx,cy),
 * warp_opt.{event_batch_size, blur_sigma}, process_opt.contrast_measure.  Uploads once; every
 * evaluation of the solve reuses it. */
int cmx_frontend_set_packet(cmx_ctx *ctx, int64_t n, const uint16_t *x, const uint16_t *y, const int64_t *t_ns,
                            int64_t t_ref_ns, double fx, double fy, double cx, double cy, int event_batch_size,
                            double blur_sigma, int contrast_measure);
int cmx_frontend_set_packet_aos(cmx_ctx *ctx, int64_t n, const void *events, const cmx_aos_layout *layout, int64_t t_ref_ns,
                                double fx, double fy, double cx, double cy, int event_batch_size, double blur_sigma,
                                int contrast_measure);

/* Packet pipeline (no reference counterpart: the CPU path has no set-up to hide).  Queues everything the packet's first
 * evaluation would otherwise do before its first vote -- destination-tile sort at omega_hint, tile-ordered bearing / dt
 * streams, chunk table -- behind the upload of cmx_frontend_set_packet[_from], and returns without waiting.  A host with
 * two contexts calls set_packet + prepare for packet k+1 on one of them BEFORE it solves packet k on the other; the GPU
 * then runs upload and sort beside the solve.  omega_hint: any estimate of the solve's
 * starting point (the previous packet's result); it affects speed only, never results. */
int cmx_frontend_prepare(cmx_ctx *ctx, const double omega_hint[3]);

/* local_contrast_fdf body: contrast (and d contrast / d omega if grad != NULL; grad == NULL is the cost-only
 * fast path used by local_contrast_f, src/frontend/local_optim_contrast_gsl.cpp:58-63). */
int cmx_frontend_eval(cmx_ctx *ctx, const double omega[3], double *contrast, double *grad /* [3] or NULL */);

/* Line-search hint (used by cmx_frontend_solve / cmx_backend_solve; available to any host whose line search knows its
 * acceptance test in advance).  Call right before a COST-ONLY evaluation: `mode` says under which condition on that
 * evaluation's value f = -contrast the gradient at the same point will be requested next -- 1: f < threshold (GSL
 * conjugate_fr's trial step: fc < fa), 2: f <= threshold (Brent loop: fm <= fb), 3: !(f >= threshold) (bracketing loop),
 * 4: always, 0: withdraw the hint.  The evaluator then queues the gradient pass behind the cost evaluation, gated on the
 * device by the cost it has just computed; a following cmx_*_eval(same parameters, grad != NULL) finds its result in flight
 * and saves one host-to-GPU turnaround (~6 us).  The hint holds for one evaluation; results never depend on it.
 * Adjoint gradient with CMX_OPT_REUSE_IMAGE and CMX_OPT_TAIL_FINALIZE on, no communicator; ignored otherwise. */
int cmx_hint_next_df(cmx_ctx *ctx, double threshold, int mode);

/* m INDEPENDENT evaluations in one call: omegas = m x 3, contrasts = m, grads = m x 3 or NULL (cost-only).  The m launch
 * chains are queued back to back and the host waits once, so the per-evaluation host round trip (~3 us of ~42) and the
 * GPU idle time behind it disappear; results are those of m cmx_frontend_eval calls.  For candidate lists (multi-start,
 * grid initialisation, finite differences) -- the line search of local_optim_contrast_gsl.cpp cannot use it, each of its
 * trial points depends on the previous cost.  Not available with a communicator attached. */
int cmx_frontend_eval_many(cmx_ctx *ctx, int m, const double *omegas, double *contrasts, double *grads);

/* exactly m calls of cmx_frontend_eval, one after the other (each waited for before the next is issued), without returning
 * to the caller in between: the evaluation pattern of the optimiser loop (local_optim_contrast_gsl.cpp:125-176) for hosts
 * whose own per-call overhead is large (an interpreter) -- replaying a recorded sequence, timing the evaluator itself. */
int cmx_frontend_eval_each(cmx_ctx *ctx, int m, const double *omegas, double *contrasts, double *grads);

/* computeImageOfWarpedEvents for display / inspection: iwe = H*W fp32 (required), deriv = H*W*3 interleaved
 * fp32 (CV_32FC3 layout) or NULL.  blur = 0 is the display overload (local_image_warped_events.cpp:41-57). */
int cmx_frontend_get_iwe(cmx_ctx *ctx, const double omega[3], int blur, float *iwe, float *deriv);

/* AngVelEstimator::publishEventImage (src/frontend/ang_vel_estimator.cpp:203-233) in one call: out = H x 2W uint8, row-major
 * ("mono8"); left half = raw events (omega = 0), right half = motion-compensated at `omega`, both blur-free -- the planes
 * cmx_frontend_get_iwe(ctx, ., 0, ., NULL) returns -- under ONE common range: with lo / hi the extremes of both halves,
 * scale = (hi - lo > DBL_EPSILON) ? 255 / (hi - lo) : 0 in fp64 (cv::normalize, NORM_MINMAX), n = S * (float)scale +
 * (float)(-lo * scale) in fp32, out = saturate_u8(round-half-to-even(255.f - n)).  A packet with no vote inside the image gives
 * 255 everywhere.  Tone map on the device; `out` may be pageable.  Like cmx_frontend_get_iwe the call leaves no evaluation point
 * resident (the next evaluation votes again) and never changes a later result. */
int cmx_frontend_render_display(cmx_ctx *ctx, const double omega[3], unsigned char *out);

/* ------------------------------------------------------------------ back end --------------------------
 * replaces PoseGraphOptimizer::copyAndUpdateTraj + EventWarper::computeImageOfWarpedEvents + computeContrast
 *   (src/backend/trajectory.cpp:240-263,501-522; src/backend/event_pano_warper.cpp:128-336;
 *    src/backend/global_focus_funcs.cpp:52-80)
 * as called from global_contrast_fdf (src/backend/global_optim_contrast_gsl_analytical.cpp:17-68). */

/* Wp x Hp panorama: fx = Wp/2pi, fy = Hp/pi (include/backend/equirectangular_camera.h:64-67). */
int cmx_backend_create(cmx_ctx **out, int device, int W, int H, const double *lut, int Wp, int Hp);

/* State PoseGraphOptimizer::processTimeWindow hands over (src/backend/pose_graph_optimizer.cpp:283-293):
 *   window events; the temp trajectory CopyAndIncrementalUpdate builds = knots [idx_cp_traj_beg_, size) of traj_
 *   with start_ns = int64(1e9*(t_beg_ + idx_cp_traj_beg_*dt_knots_)) (cmx_traj_temp_start_ns) and dt_ns;
 *   order = 2 (linear, So3Spline<2>) or 4 (cubic, So3Spline<4>); num_fixed = idx_cp_opt_beg_ - idx_cp_traj_beg_;
 *   t_next_win_beg = t_win_beg_ + win_stride_; warp_opt_.{event_batch_size, event_sample_rate, blur_sigma};
 *   IG = the persistent global map (Hp*Wp fp32) or NULL for an all-zero map.  Also performs setFirstIter(true):
 *   alpha is recomputed by the first evaluation of the window (event_pano_warper.cpp:201-210). */
int cmx_backend_set_window(cmx_ctx *ctx, int64_t n, const uint16_t *x, const uint16_t *y, const int64_t *t_ns,
                           int order, int K, const double *knots_xyzw, int64_t start_ns, int64_t dt_ns,
                           int num_fixed, int64_t t_next_win_beg_ns, int event_batch_size, int event_sample_rate,
                           double blur_sigma, int contrast_measure, const float *IG);
int cmx_backend_set_window_aos(cmx_ctx *ctx, int64_t n, const void *events, const cmx_aos_layout *layout, int order, int K,
                               const double *knots_xyzw, int64_t start_ns, int64_t dt_ns, int num_fixed, int64_t t_next_win_beg_ns,
                               int event_batch_size, int event_sample_rate, double blur_sigma, int contrast_measure, const float *IG);

/* Window pipeline: the back end's counterpart of cmx_frontend_prepare -- pose table at drotv_hint (NULL = zero increments),
 * destination-tile sort, chunk table and bearing streams of the window handed over last, queued without waiting. */
int cmx_backend_prepare(cmx_ctx *ctx, const double *drotv_hint /* [3*(K-num_fixed)] or NULL */);

/* global_contrast_fdf body: drotv = 3*(K-num_fixed) incremental rotation vectors applied by LEFT
 * multiplication to the non-fixed knots (trajectory.cpp:236 / :497); grad has the same length or is NULL. */
int cmx_backend_eval(cmx_ctx *ctx, const double *drotv, double *contrast, double *grad);

/* m independent evaluations in one call (see cmx_frontend_eval_many): drotvs = m x 3(K-num_fixed), grads likewise or NULL */
int cmx_backend_eval_many(cmx_ctx *ctx, int m, const double *drotvs, double *contrasts, double *grads);
/* m calls of cmx_backend_eval, one after the other (see cmx_frontend_eval_each) */
int cmx_backend_eval_each(cmx_ctx *ctx, int m, const double *drotvs, double *contrasts, double *grads);

enum { CMX_PLANE_IL_OLD = 0, CMX_PLANE_IL_NEW = 1, CMX_PLANE_IWE = 2, CMX_PLANE_DERIV0 = 16 };
/* planes of the LAST evaluation (what updateIG / publishEventImage read, event_pano_warper.cpp:109-126):
 * IL_old / IL_new are raw; IWE is the blurred I = IL + alpha*IGp; CMX_PLANE_DERIV0+j is blurred derivative
 * plane j (only after an evaluation with CMX_GRAD_PLANES and grad != NULL). host: Hp*Wp fp32. */
int cmx_backend_get_plane(cmx_ctx *ctx, int which, float *host);
int cmx_backend_get_alpha(cmx_ctx *ctx, double *alpha);
/* Parity read-back of the per-batch pose table the splat and gather kernels read (be_pose_table kernels = So3Spline::evaluate
 * with Jacobians, thirdparty/basalt-headers/include/basalt/spline/so3_spline.h:218-274, as Trajectory::evaluate stores them,
 * src/backend/trajectory.cpp:86-110 / :329-355): recomputed on the device at the LAST evaluation's parameters (zero increments
 * before the first one).  R = n x 9 fp64 row-major; Jcp = n x 36 fp32, the 3 x 3*order row-major block in front; idx = first
 * control pose of the batch's segment; t_batch_ns = the batch's pose time.  Any output may be NULL; *n_batches = batches of
 * the window; at most max_batches rows are written. */
int cmx_backend_get_pose_table(cmx_ctx *ctx, int max_batches, double *R, float *Jcp, int *idx, int64_t *t_batch_ns, int *n_batches);

/* Global-map upkeep on the device (once per window, after the solve).  Keeps IG_ and
 * IG_update_times_map_ resident across windows: pass IG = CMX_KEEP_MAP to cmx_backend_set_window instead of
 * round-tripping a 4..32 MB plane through the host every window.
 *   cmx_backend_update_map    EventWarper::updateIG          (src/backend/event_pano_warper.cpp:109-126): IG += IL_old of
 *                             the LAST evaluation wherever the visit count is <= max_update_times
 *   cmx_backend_mark_visited  EventWarper::setUpdateTimesIG  (:81-107) for one pose (the caller loops over the poses
 *                             every 0.05 s, src/backend/pose_graph_optimizer.cpp:325-337); counts saturate at 255
 *   cmx_backend_reset_map     resetIG + zero visit counts;   get/set_map: host copies (either pointer may be NULL) */
#define CMX_KEEP_MAP ((const float *)(uintptr_t)1)
int cmx_backend_update_map(cmx_ctx *ctx, int max_update_times);
int cmx_backend_mark_visited(cmx_ctx *ctx, const double quat_xyzw[4], int radius);
int cmx_backend_reset_map(cmx_ctx *ctx);
int cmx_backend_get_map(cmx_ctx *ctx, float *IG, unsigned char *visits);
int cmx_backend_set_map(cmx_ctx *ctx, const float *IG, const unsigned char *visits);
/* PoseGraphOptimizer::publishEventImage (src/backend/pose_graph_optimizer.cpp:378-413) on the RESIDENT map IG, in one call:
 *   v = normalize(IG, 0, 1, NORM_MINMAX);  p = |v|^gamma (cv::pow; gamma = 1 copies);  q = normalize(p, 0, 255, NORM_MINMAX) as
 *   8 bits (round half to even, saturated; the extremes of p are the images of the extremes of v);  out = 255 - q.
 * fov_quat_xyzw == NULL: out = Hp x Wp uint8 ("mono8").  Otherwise out = Hp x Wp x 3 uint8 ("bgr8"): three equal channels, then
 * EventWarper::drawSensorFOV (src/backend/event_pano_warper.cpp:56-79) for that pose: every sensor border pixel is warped to the
 * panorama, its coordinates rounded half to even (cv::Point2d -> cv::Point) and (B, G, R) = (255, 0, 0) written there.  Border
 * pixels that land outside the panorama are skipped (the reference writes them out of bounds).  A blank or constant map gives
 * 255 everywhere.  gamma must be finite and > 0, the quaternion non-zero (it is normalised).  Valid right after
 * cmx_backend_create; needs no window and touches no evaluation state.  On a group handle it reads member 0. */
int cmx_backend_render_map(cmx_ctx *ctx, double gamma, const double fov_quat_xyzw[4] /* or NULL */, unsigned char *out);
/* int64_t(1e9 * (t_beg + idx_traj_beg*dt_knots)) -- the (double)->ns truncation of trajectory.cpp:255-256 */
int64_t cmx_traj_temp_start_ns(double t_beg, int idx_traj_beg, double dt_knots);

/* ------------------------------------------------------------------ device-resident event store -----------
 * SURVEY.md section 8f rank 3.  The reference keeps the stream in AngVelEstimator::events_ and copies a packet
 * (src/frontend/ang_vel_estimator.cpp:137-147) or a window (src/backend/pose_graph_optimizer.cpp:131-165) out of it for
 * every solve; consecutive packets and windows overlap heavily.  With a store the stream is uploaded ONCE
 * (cmx_events_push as events arrive), packets / windows are cut from it on the device by global event index, and
 * cmx_events_drop_before is deleteOldEvents (ang_vel_estimator.cpp:149-173).  Results are identical to
 * cmx_frontend_set_packet / cmx_backend_set_window on the same events.  One store per GPU, shared by the front-end and
 * back-end contexts of that GPU; not thread-safe (serialise push/drop against set_*_from, as the reference does with
 * mutex_events).
 * cmx_events_create_group: ONE store with a replica of the stream on every distinct device of a group's member list (the list
 * given to cmx_backend_create_group): cmx_events_push packs once on the host and uploads to all replicas side by side,
 * cmx_events_drop_before compacts all of them, cmx_backend_set_window_from on the group's handle lets every member cut ITS
 * batch range on its own device (no event crosses the host at hand-over), and any front-end / back-end context on one of
 * those devices can cut from it too.  cmx_events_devices lists the replicas' devices (returns their number).
 * Polarity.  cmx_events_push_pol / _push_aos_pol store one polarity byte per event (0 = OFF, 1 = ON; any nonzero input is ON) in
 * an array of its own beside the coordinates and timestamps, on every replica, allocated by the first such push and compacted by
 * cmx_events_drop_before like the other two.  A store holds polarity for ALL of its events or for none: the first push into an
 * empty store decides, and the other form of push into a non-empty store returns CMX_ERR_STATE and pushes nothing.  A store that
 * never saw a _pol push allocates and copies exactly what it did before these calls existed.  The only reader of the bytes is
 * cmx_backend_recon_pol_add_from: packets, windows, recon_add_from, bind_from and warp_from cut from a store with polarity get
 * the same bits as from one without.  cmx_events_has_polarity: 1 when the events held carry polarity, else 0 (an empty store: 0). */
typedef struct cmx_events cmx_events;
int cmx_events_create(cmx_events **out, int device, int W, int H, size_t capacity);
int cmx_events_create_group(cmx_events **out, const int *devices, int n_devices, int W, int H, size_t capacity);
int cmx_events_devices(const cmx_events *ev, int *devices, int max_devices);
void cmx_events_destroy(cmx_events *ev);
const char *cmx_events_last_error(const cmx_events *ev);
int cmx_events_push(cmx_events *ev, int64_t n, const uint16_t *x, const uint16_t *y, const int64_t *t_ns);
int cmx_events_push_aos(cmx_events *ev, int64_t n, const void *events, const cmx_aos_layout *layout); /* e.g. msg->events.data() */
int cmx_events_push_pol(cmx_events *ev, int64_t n, const uint16_t *x, const uint16_t *y, const int64_t *t_ns, const uint8_t *pol);
int cmx_events_push_aos_pol(cmx_events *ev, int64_t n, const void *events, const cmx_aos_layout *layout, size_t off_polarity);
int cmx_events_has_polarity(const cmx_events *ev);
int cmx_events_drop_before(cmx_events *ev, int64_t global_index);
int64_t cmx_events_begin(const cmx_events *ev); /* global index of the oldest event held */
int64_t cmx_events_end(const cmx_events *ev);   /* one past the newest */
/* Selection on the device: a STABLE stream compaction from a range of one store into another store -- what acts on the scores and
 * flags of cmx_backend_recon_score_from_device (outlier rejection, hot-pixel removal) without the events leaving the device.  The
 * result is an ordinary store: packets, windows, recon_add_from, bind_from, bind_append_from, warp_from, score_from, pol_add_from,
 * views, voxels and surfaces read it by (store, first, count) like any other.
 *   select      An event of src[first, first + count) is kept when EVERY criterion that is given (non-NULL) holds:
 *                 keep        count bytes, nonzero = keep
 *                 score       count floats, keep when score >= min_score, compared in fp32 (a NaN score is dropped)
 *                 flags       count bytes, keep when (flags & flags_mask) == flags_value (the export's bit pair: mask = value = 3,
 *                             "the event voted")
 *                 pixel_keep  W*H bytes at y*W+x, nonzero = the events of this pixel are kept
 *               With every pointer NULL everything is kept: a device-side store-to-store copy.  cmx_select::size = sizeof(cmx_select).
 *               The kept events are APPENDED to dst in their source order (equal timestamps keep their order; dst stays
 *               time-sorted); *n_kept (may be NULL) = their number.  Afterwards dst is indistinguishable from a store into which the
 *               same events were pushed from host arrays: packed words, timestamps, polarity bytes, the host mirror of the
 *               timestamps.  src is read only.  An empty dst takes src's polarity form, as the first push does.
 *               Synchronous: the work runs on dst's own stream and the call returns when dst is complete.  select takes host
 *               arrays (uploaded into scratch of dst); select_device takes device pointers on the stores' device for every non-NULL
 *               member, and work of the caller's that still writes them must be finished (the rule of recon_warp_from_device).
 *               Three launches -- predicate + per-tile count, scan of the tile counts, scatter -- and the host reads the total in
 *               between: the scatter runs only when everything fits.
 *   errors      each leaves dst exactly as it was (begin, end, contents).  CMX_ERR_INVALID_ARG: dst == src, a NULL store, sel NULL or
 *               sel->size not the struct's; W / H differ; a range src does not hold; either store has more than one replica (group
 *               stores are out of scope) or the two are on different devices; dst->size + kept > capacity ("event store full").
 *               CMX_ERR_STATE: dst is non-empty and its polarity form differs from src's.  CMX_ERR_TIME_ORDER: the first KEPT event
 *               is earlier than dst's last event.
 *   pixel_counts  counts[y*W+x] = the number of events of the range at that pixel: W*H words, written, not accumulated (count == 0:
 *               all zero); exact for any distribution (one integer atomic per event).  _device: d_counts on the store's device.
 *               Synchronous, on the store's stream.  A group store: its first replica.
 *   read        the inverse of cmx_events_push_pol: x, y unpacked from the packed words, pol 0 / 1.  Any of x, y, t_ns may be NULL;
 *               pol is NULL or count bytes (CMX_ERR_STATE when the store holds no polarity).  A test and export call, sliced through
 *               the store's pinned staging.
 *   threads     pixel_counts* and read take a const store but use its stream, its pinned staging and its error text: like every
 *               other call on a store they are not thread-safe against each other or against push, drop_before or select on the
 *               same store (as source or destination). */
typedef struct {
  size_t size;                     /* sizeof(cmx_select): lets the struct grow without an ABI bump */
  const unsigned char *keep;       /* count bytes or NULL: nonzero = keep */
  const float *score;              /* count floats or NULL: keep when score >= min_score in fp32 (NaN: dropped) */
  float min_score;
  const unsigned char *flags;      /* count bytes or NULL: keep when (flags & flags_mask) == flags_value */
  unsigned char flags_mask, flags_value;
  const unsigned char *pixel_keep; /* W*H bytes at y*W+x or NULL: nonzero = events of this pixel are kept */
} cmx_select;
int cmx_events_select(cmx_events *dst, const cmx_events *src, int64_t first, int64_t count, const cmx_select *sel, int64_t *n_kept);
int cmx_events_select_device(cmx_events *dst, const cmx_events *src, int64_t first, int64_t count, const cmx_select *sel,
                             int64_t *n_kept);
int cmx_events_pixel_counts(const cmx_events *ev, int64_t first, int64_t count, uint32_t *counts);
int cmx_events_pixel_counts_device(const cmx_events *ev, int64_t first, int64_t count, uint32_t *d_counts);
int cmx_events_read(const cmx_events *ev, int64_t first, int64_t count, uint16_t *x, uint16_t *y, int64_t *t_ns, unsigned char *pol);
int cmx_frontend_set_packet_from(cmx_ctx *ctx, const cmx_events *ev, int64_t first, int64_t count, int64_t t_ref_ns,
                                 double fx, double fy, double cx, double cy, int event_batch_size, double blur_sigma,
                                 int contrast_measure);
int cmx_backend_set_window_from(cmx_ctx *ctx, const cmx_events *ev, int64_t first, int64_t count, int order, int K,
                                const double *knots_xyzw, int64_t start_ns, int64_t dt_ns, int num_fixed,
                                int64_t t_next_win_beg_ns, int event_batch_size, int event_sample_rate,
                                double blur_sigma, int contrast_measure, const float *IG);

/* ------------------------------------------------------------------ whole-trajectory reconstruction ---------
 * The panorama of ALL events warped along the FINAL refined trajectory -- the product a rotational event SLAM is run for.
 * cmx_backend_set_window takes at most 64 control poses (one bundle-adjustment window); these calls take a spline of ANY knot
 * count (the knots live in device memory; at least 2^20 of them, 32 bytes each) and accumulate into a plane of their own:
 *     recon_begin(trajectory)   recon_add*(events) ...   recon_get / recon_render (any number of times)   recon_end
 * They act on an ordinary back-end context (cmx_backend_create) and never change a later evaluation: the window, the resident
 * evaluation point, IG, the visit counts and the exchange sets are left alone.  On a group handle every one of them returns
 * CMX_ERR_STATE; add / get / render before begin return CMX_ERR_STATE, end without begin is CMX_OK.
 *   begin   order = 2 | 4, K >= order knots (copied to the device), start_ns / dt_ns as in cmx_backend_set_window, batch size at most
 *           2^30 (CMX_ERR_INVALID_ARG above it: a slice is at least one batch and is indexed with 32-bit integers); zeroes the plane
 *           and both counters; records batch size, sample rate and the value of CMX_OPT_DETERMINISTIC at this moment.  A second begin
 *           starts over.
 *   add*    ONE call = the vote loop of EventWarper::computeImageOfWarpedEvents (src/backend/event_pano_warper.cpp:188-196, :233-311)
 *           over exactly the events handed in, ADDED to the plane: batches start at the call's first event, a trailing batch holding
 *           a single event is skipped, the batch pose is taken at the batch time cmx_backend_set_window uses, sampling restarts at
 *           every batch start, and an event votes when 1 <= xx < Wp-2 && 1 <= yy < Hp-2 whatever its time (no old / new split, no
 *           alpha, no IG, no blur).  add(A) then add(B) therefore equals the sum of two separate loops, and equals the loop over
 *           A || B exactly when len(A) is a multiple of the batch size.  Checks and status codes are those of
 *           cmx_backend_set_window[_aos|_from]: CMX_ERR_INVALID_ARG, CMX_ERR_EVENT_RANGE, CMX_ERR_TIME_ORDER, CMX_ERR_SPLINE_RANGE,
 *           with one rule stated more strictly: on the host paths EVERY event handed in must lie inside the sensor, at every
 *           sample rate -- the events the sampling skips and a skipped trailing event included (cmx_backend_set_window looks at
 *           events it does not pack only when it sub-samples: at rate 1 it lets a skipped trailing event pass unseen).
 *           All of this is validated before the first vote, so a call that fails VALIDATION adds nothing.  A runtime failure
 *           (CMX_ERR_HIP: an allocation, a copy or a launch refused in the middle of a long input) is outside that promise:
 *           slices queued before it have voted, and the reconstruction should be begun again.
 *           n may be anything up to the event limit: long inputs are processed in internal slices of whole batches (packing and
 *           upload of one slice beside the vote kernel of the one before), staging memory does not grow with n.
 *   get     pano = Hp*Wp fp32 or NULL (counters only); *n_sampled = events the sampling selected so far (exact), *n_inside = events
 *           that voted so far; either may be NULL.  Accumulation may continue afterwards.
 *   render  cmx_backend_render_map's tone map, argument rules and output (mono8, or bgr8 with the sensor outline) on this plane.
 *   end     frees the plane(s), the knots and the staging.
 * CMX_OPT_DETERMINISTIC = 1 at begin: votes are 64-bit integer adds into a 2^-30 fixed-point plane (get / render convert to fp32):
 * bitwise identical from run to run, for any slicing of the same events at batch multiples, and through the three ingest paths.
 * Otherwise votes are fp32 atomics: equal up to summation order. */
int cmx_backend_recon_begin(cmx_ctx *ctx, int order, int K, const double *knots_xyzw, int64_t start_ns, int64_t dt_ns,
                            int event_batch_size, int event_sample_rate);
int cmx_backend_recon_add(cmx_ctx *ctx, int64_t n, const uint16_t *x, const uint16_t *y, const int64_t *t_ns);
int cmx_backend_recon_add_aos(cmx_ctx *ctx, int64_t n, const void *events, const cmx_aos_layout *layout);
int cmx_backend_recon_add_from(cmx_ctx *ctx, const cmx_events *ev, int64_t first, int64_t count);
int cmx_backend_recon_get(cmx_ctx *ctx, float *pano /* Hp*Wp or NULL */, int64_t *n_sampled, int64_t *n_inside /* either may be NULL */);
int cmx_backend_recon_render(cmx_ctx *ctx, double gamma, const double fov_quat_xyzw[4] /* or NULL */, unsigned char *out);
int cmx_backend_recon_end(cmx_ctx *ctx);
/* Per-event export: WHERE every event lands under the trajectory the reconstruction holds -- what a host needs for any product other
 * than the count panorama (the signed polarity map, pinhole frames or crops, voxel grids, time surfaces and support scores for
 * outlier flags have calls of their own, cmx_backend_recon_pol_*, _view_*, _voxel_*, _surface_* and _score*): the export itself
 * never reads polarity, the host joins the entries with whatever it kept.
 *   output   ONE entry per event handed in, sampled or not, in input order: xy_out[2i], xy_out[2i+1] = (px, py), flags_out[i]
 *            (flags_out may be NULL).  CMX_WARP_F64: 2 doubles per event; CMX_WARP_F32: 2 floats, (float)px and (float)py.
 *   poses    spline, batch size and sample rate are those of recon_begin / restart / extend; the knots are the ones the
 *            reconstruction holds NOW (e.g. the result of recon_solve).  Batches start at the call's first event, exactly as in
 *            add*: event i belongs to batch b = i / B and is warped with that batch's pose at the batch time add* uses.  (px, py)
 *            is the fp64 panorama coordinate the vote kernels take their cell xx = (int)px and weight dx = (float)(px - xx) from --
 *            the same device functions, so the same bits.  With event_batch_size = 1 every event gets the pose at its own time.
 *   the lone trailing event   add* skips a trailing batch of exactly one event.  The export warps that event with the pose at its
 *            OWN timestamp and clears its SAMPLED bit.  Its time is validated against the spline like a batch time
 *            (CMX_ERR_SPLINE_RANGE): the one place where warp* is stricter than add*.
 *   flags    CMX_WARP_SAMPLED: (i - b*B) % rate == 0 and the event is not the lone trailing one -- exactly the events add* reads.
 *            CMX_WARP_INSIDE: 1 <= xx < Wp-2 && 1 <= yy < Hp-2.  flags == 3: this event voted in add*.
 *   state    read-only on the reconstruction: the plane, the counters, the knots, an open gradient pass, a binding, a frozen head
 *            and a released head are untouched, and so are the window, IG and the exchange sets.  Works after release_head (only
 *            the knots are read).
 *   status   validation and status codes of add* / add_from, complete before anything is written: a call that fails validation
 *            writes nothing to the outputs.  CMX_ERR_STATE before begin and on a group handle; CMX_ERR_INVALID_ARG for an unknown
 *            format or a NULL xy_out with n > 0; n == 0 is valid.
 *   long inputs run in the internal slices of whole batches of add*; staging memory does not grow with n.  Host output: the kernel of
 *            slice k writes device staging, a copy on a stream of its own moves it to pinned memory, and host threads copy it into
 *            the caller's arrays while slice k+1 runs.  _from_device writes straight into device pointers on the context's device
 *            (no staging; any alignment of the element type works, one store per pair needs d_xy_out 16- / 8-byte aligned). */
#define CMX_WARP_F64 0          /* xy_out: 2 doubles per event (px, py) */
#define CMX_WARP_F32 1          /* xy_out: 2 floats per event: (float)px, (float)py */
#define CMX_WARP_SAMPLED 1      /* flag bit 0 */
#define CMX_WARP_INSIDE  2      /* flag bit 1 */
int cmx_backend_recon_warp(cmx_ctx *ctx, int64_t n, const uint16_t *x, const uint16_t *y, const int64_t *t_ns, int format, void *xy_out,
                           unsigned char *flags_out /* n bytes or NULL */);
int cmx_backend_recon_warp_aos(cmx_ctx *ctx, int64_t n, const void *events, const cmx_aos_layout *layout, int format, void *xy_out,
                               unsigned char *flags_out);
int cmx_backend_recon_warp_from(cmx_ctx *ctx, const cmx_events *ev, int64_t first, int64_t count, int format, void *xy_out,
                                unsigned char *flags_out);
int cmx_backend_recon_warp_from_device(cmx_ctx *ctx, const cmx_events *ev, int64_t first, int64_t count, int format, void *d_xy_out,
                                       unsigned char *d_flags_out /* device pointers on the context's device */);
/* Per-event support scores: the way back from the map to the events -- the motion-compensated image read at the place where an event
 * lands, with or without the event's own vote.  Events on a sharp edge of the panorama have many companions, noise events and hot
 * pixels have none: outlier flags, denoising, an input weight beside the voxel grids and time surfaces.  On an open reconstruction:
 *     recon_add* ...   recon_score_open(sigma)   recon_score*(events, loo) (any number of times)   [recon_score_plane]
 *   the plane   is the count panorama of recon_add* / eval_from / eval_bound as it stands at score_open.
 *   S           the support plane: GaussianBlur(plane, blur_sigma) exactly as recon_contrast forms it (the same taps, REFLECT_101, the
 *               same operation order); with blur_sigma == 0 the plane itself.  In deterministic mode S comes from the fp32 view of the
 *               fixed-point plane (what recon_get returns).
 *   score       event i is warped exactly as recon_warp* warps it: cell (xx, yy) = ((int)px, (int)py), fp32 fractions dx, dy, and the
 *               four fp32 weights of the vote, each a single rounded product: w00 = (1-dx)(1-dy), w01 = dx(1-dy), w10 = (1-dx)dy,
 *               w11 = dx dy.  If INSIDE,
 *                   score_i = ((w00 S[yy][xx] + w01 S[yy][xx+1]) + w10 S[yy+1][xx]) + w11 S[yy+1][xx+1]
 *               in fp32, every product and every sum rounded on its own, in this order, no FMA: a host reproduces it bit for bit
 *               from recon_score_plane and the (px, py) of recon_warp*.  Otherwise 0.0f.
 *   loo != 0    leave-one-out: an event with flags == 3 (SAMPLED | INSIDE) voted into the plane, and what S hands back of its own four
 *               adds is subtracted, score_i - self_i in one fp32 subtraction:
 *                   self_i = (sum_{j,j'} wx_j wx_j' Gx[xx+j, xx+j']) * (the same in y),   wx = (1-dx, dx), wy = (1-dy, dy)
 *               with Gx[a, b] the entry of the 1-D REFLECT_101 filter matrix: the tap g(a-b) plus every tap that folds onto b at the
 *               left or the right border.  blur_sigma == 0: self_i = ((w00^2 + w01^2) + w10^2) + w11^2.  Events that are not SAMPLED,
 *               and the lone trailing event, did not vote: nothing is subtracted.  NO clamp at zero: in default mode the plane is a sum
 *               of fp32 atomics, so a leave-one-out score of -1e-7 is honest; in deterministic mode |.| <= 2^-28 for an event alone
 *               in its cells (2^-30 per vote, four cells).  The subtraction is right for events that DID vote into this plane: score
 *               the events that were added, in the cuts they were added in.
 *   score_open  takes the snapshot: S is formed from the plane as accumulated NOW.  Accepts every blur_sigma recon_contrast accepts
 *               (CMX_ERR_INVALID_ARG: not finite, radius > 12) and needs Wp > 2r+1 && Hp > 2r+1 (CMX_ERR_INVALID_ARG: the own
 *               contribution folds single reflections, as the adjoint gradient does).  The taps are those of recon_contrast: an open
 *               gradient pass at ANOTHER sigma is closed exactly as recon_contrast(sigma) would close it, one at the same sigma is
 *               left alone.  The pass stays open until something changes the plane or the knots: begin, restart, extend, every add*
 *               that votes into the count plane, eval_from, eval_bound, solve, bind*, freeze_head, advance_head, end.  pol_add*,
 *               view_*, voxel_*, surface_*, warp*, grad_add*, contrast, get and render do not close it.
 *   score*      CMX_ERR_STATE without an open pass, before begin and on a group handle.  Otherwise everything of recon_warp*: one
 *               float per event handed in, in input order; the same flags (flags_out may be NULL); the same batches and batch times;
 *               the lone trailing event scored with the pose at its own time, its time validated against the spline; validation and
 *               status codes complete before anything is written; n == 0 is valid, a NULL score_out with n > 0 is
 *               CMX_ERR_INVALID_ARG; the internal slices and the double-buffered device staging -> pinned -> caller path of the host
 *               outputs; _from_device writes straight into device pointers on the context's device.  Read-only on everything but S:
 *               the plane, the counters, the knots, an open gradient pass, a binding, a frozen or released head, the target sets, the
 *               window, IG and the exchange sets are untouched.  Works after release_head.
 *   score_plane copies S out (tests, display).  CMX_ERR_STATE without an open pass. */
int cmx_backend_recon_score_open(cmx_ctx *ctx, double blur_sigma);
int cmx_backend_recon_score_plane(cmx_ctx *ctx, float *S /* Hp*Wp */);
int cmx_backend_recon_score(cmx_ctx *ctx, int64_t n, const uint16_t *x, const uint16_t *y, const int64_t *t_ns, int loo, float *score_out,
                            unsigned char *flags_out /* n bytes or NULL */);
int cmx_backend_recon_score_aos(cmx_ctx *ctx, int64_t n, const void *events, const cmx_aos_layout *layout, int loo, float *score_out,
                                unsigned char *flags_out);
int cmx_backend_recon_score_from(cmx_ctx *ctx, const cmx_events *ev, int64_t first, int64_t count, int loo, float *score_out,
                                 unsigned char *flags_out);
int cmx_backend_recon_score_from_device(cmx_ctx *ctx, const cmx_events *ev, int64_t first, int64_t count, int loo, float *d_score_out,
                                        unsigned char *d_flags_out /* device pointers on the context's device */);
/* Signed polarity panorama: the ON and the OFF events of the recording as two planes, ON - OFF being the map that feeds intensity
 * reconstruction and the usual red / blue picture.  On an open reconstruction:
 *     recon_pol_add*(events, polarity) ...   recon_pol_get / recon_pol_render (any number of times)   [recon_pol_reset]
 *   pol_add*   ONE call = the vote loop of add* over exactly the events handed in -- the same batches and batch times, sampling
 *              restarting at every batch start, the lone trailing event skipped, the same vote test, cell and weights (the same
 *              device functions) -- with ONE difference: an event with polarity != 0 votes into the ON plane, any other into the OFF
 *              plane.  Polarity: pol[i] (one byte per event), the byte at off_polarity of record i (CMX_AOS_DVS_POLARITY for
 *              dvs_msgs::Event), or the store's own (pol_add_from: CMX_ERR_STATE when the store holds none).  Validation and status
 *              codes are add*'s, complete before the first vote: a call that fails validation adds nothing to either plane.
 *   planes     two Hp*Wp planes (and their 2^-30 fixed-point twins when CMX_OPT_DETERMINISTIC was 1 at begin: bitwise reproducible,
 *              for any slicing at batch multiples and through every ingest path), allocated by the first pol_add*.  begin, restart
 *              and pol_reset clear them -- votes under other knots are stale -- and end frees them.  EVERY other call leaves them
 *              alone, extend, eval_bound and recon_solve included, although they move the knots: call pol_reset before voting anew.
 *   state      the count plane of add*, its counters, an open gradient pass, a binding, a frozen or released head, the window, IG
 *              and the exchange sets are neither read nor written: the calls work with a gradient pass open, with events bound,
 *              after freeze_head and after release_head (only the knots are read).
 *   pol_get    on / off = Hp*Wp fp32 each or NULL; *n_on / *n_off = events that voted into each plane so far; either may be NULL.
 *              Before the first pol_add*: zeros.
 *   pol_render one device pass over s = ON - OFF: m = max |s| (m == 0: the neutral image), v = sign(s) (|s| / m)^gamma in fp32;
 *              CMX_POL_MONO8: out = Hp*Wp bytes, rint(127.5f + 127.5f v) -- OFF dark, ON bright, no votes 128;
 *              CMX_POL_BGR8: out = Hp*Wp*3 bytes on white, a = rint(255 |v|): an ON pixel is (B, G, R) = (255 - a, 255 - a, 255),
 *              an OFF pixel (255, 255 - a, 255 - a).  Any other mode, gamma <= 0 or not finite: CMX_ERR_INVALID_ARG.
 *   pol_reset  clears the two planes and their counters, nothing else.
 * All of them return CMX_ERR_STATE before begin and on a group handle. */
#define CMX_POL_MONO8 0
#define CMX_POL_BGR8  1
int cmx_backend_recon_pol_add(cmx_ctx *ctx, int64_t n, const uint16_t *x, const uint16_t *y, const int64_t *t_ns, const uint8_t *pol);
int cmx_backend_recon_pol_add_aos(cmx_ctx *ctx, int64_t n, const void *events, const cmx_aos_layout *layout, size_t off_polarity);
int cmx_backend_recon_pol_add_from(cmx_ctx *ctx, const cmx_events *ev, int64_t first, int64_t count);
int cmx_backend_recon_pol_get(cmx_ctx *ctx, float *on, float *off /* Hp*Wp each, either may be NULL */, int64_t *n_on, int64_t *n_off);
int cmx_backend_recon_pol_render(cmx_ctx *ctx, double gamma, int mode, unsigned char *out);
int cmx_backend_recon_pol_reset(cmx_ctx *ctx);
/* Pinhole views: motion-compensated event frames and zoomed crops.  A set of M virtual pinhole cameras is attached to an open
 * reconstruction; one vote pass warps every sampled event ONCE into the world frame with the trajectory the reconstruction holds and
 * votes it into every view whose time range holds the event's batch time.  A video of de-rotated frames is M views with disjoint
 * ranges and the spline's pose at each slice centre; a crop is one view over all time with a longer focal length.
 *     recon_view_begin(views)   recon_view_add*(events) ...   recon_view_get / recon_view_render (any number of times)
 *     [recon_view_reset]   recon_view_end
 *   view_begin needs an open reconstruction.  Copies the views to the device -- R(quat)^T formed on the host in fp64 from the
 *              normalised quaternion -- allocates n_views fp32 planes of Wv x Hv (and their 2^-30 fixed-point twins when
 *              CMX_OPT_DETERMINISTIC was 1 at recon_begin) and zeroes them and one vote counter per view.  A second view_begin starts
 *              over.  CMX_ERR_INVALID_ARG: Wv or Hv outside [4, 8192]; n_views outside [1, 4096]; n_views * Wv * Hv > 2^28; a
 *              quaternion that is zero or not finite; fx or fy not finite or <= 0; cx or cy not finite; t_lo_ns >= t_hi_ns.  Time
 *              ranges may overlap, nest or leave gaps, and the views need not be ordered.
 *   view_add*  ONE call = the vote loop of add* over exactly the events handed in -- the same batches and batch times, sampling
 *              restarting at every batch start, the lone trailing event skipped, the same validation and status codes, complete
 *              before the first vote: a call that fails validation adds nothing to any plane.  Per sampled event, in fp64:
 *                  ray_w = R_batch * bearing                      (the vote kernels' own function and pose: the same bits)
 *                  for every view with t_lo_ns <= batch time < t_hi_ns:
 *                      v = R(quat)^T ray_w,   iz = 1 / v.z,   u = fx (v.x iz) + cx,   w = fy (v.y iz) + cy
 *                      the vote test, in floating point BEFORE any conversion:  v.z > 0 && 1 <= u < Wv-2 && 1 <= w < Hv-2
 *                      (a NaN fails it, and no value outside the plane is ever cast to an integer)
 *                      xx = (int)u, dx = (float)(u - xx), yy = (int)w, dy = (float)(w - yy): the four bilinear adds of add* into
 *                      that view's plane (64-bit integer adds into its fixed-point twin in deterministic mode), and one count
 *              Cost per event grows with the views that hold its batch time, not with n_views.
 *   view_get   planes = count * Hv*Wv fp32 or NULL, n_voted = count counters or NULL, for views [first_view, first_view + count);
 *              CMX_ERR_INVALID_ARG when the range leaves the set.  Accumulation may continue afterwards.
 *   view_render  cmx_backend_recon_render's tone map and gamma rules, without the outline, on ONE view's plane: out = Hv*Wv mono8.
 *   view_reset clears the planes and the counters and keeps the views.   view_end frees the set (without a set: CMX_OK).
 *   state      the calls read the knots the reconstruction holds NOW and nothing else of it, and write only the view planes and
 *              their counters: the count plane of add*, its counters, the polarity planes, an open gradient pass, a binding, a frozen
 *              or released head, the window, IG and the exchange sets are untouched, and the calls work with a gradient pass open,
 *              with events bound, after freeze_head and after release_head.  recon_begin and recon_end free the view set; restart and
 *              view_reset clear planes and counters and keep the views.  EVERY other call leaves them alone, extend, eval_bound and
 *              recon_solve included, although they move the knots: call view_reset before voting anew.
 *   status     CMX_ERR_STATE before recon_begin, before view_begin (add*, get, render, reset) and on a group handle.
 * Deterministic mode: every plane is a sum of integers -- bitwise identical from run to run, for any slicing at batch multiples,
 * through the three ingest paths, and whatever other views are in the set.  Otherwise votes are fp32 atomics. */
typedef struct cmx_recon_view {
  double  quat_xyzw[4];      /* camera orientation in the spline's world frame: ray_cam = R(quat)^T ray_world */
  double  fx, fy, cx, cy;    /* pinhole intrinsics of the view, in view pixels */
  int64_t t_lo_ns, t_hi_ns;  /* a batch votes into this view when t_lo_ns <= batch time < t_hi_ns */
} cmx_recon_view;
int cmx_backend_recon_view_begin(cmx_ctx *ctx, int Wv, int Hv, int n_views, const cmx_recon_view *views);
int cmx_backend_recon_view_add(cmx_ctx *ctx, int64_t n, const uint16_t *x, const uint16_t *y, const int64_t *t_ns);
int cmx_backend_recon_view_add_aos(cmx_ctx *ctx, int64_t n, const void *events, const cmx_aos_layout *layout);
int cmx_backend_recon_view_add_from(cmx_ctx *ctx, const cmx_events *ev, int64_t first, int64_t count);
int cmx_backend_recon_view_get(cmx_ctx *ctx, int first_view, int count, float *planes /* count*Hv*Wv or NULL */,
                               int64_t *n_voted /* count or NULL */);
int cmx_backend_recon_view_render(cmx_ctx *ctx, int view, double gamma, unsigned char *out /* Hv*Wv mono8 */);
int cmx_backend_recon_view_reset(cmx_ctx *ctx);
int cmx_backend_recon_view_end(cmx_ctx *ctx);
/* Voxel grids: the discretised event volume event-based networks read, motion-compensated.  A set of G grids is attached to an open
 * reconstruction; a grid is a cmx_recon_view -- orientation, intrinsics, [t_lo_ns, t_hi_ns) -- with n_bins time bins over its range
 * (trajectory.frame_views' output can be passed as it is).  One vote pass warps every sampled event ONCE into the world frame and
 * spreads it over four pixels bilinearly and over its two neighbouring bins with triangular weights, signed by polarity.
 *     recon_voxel_begin(grids)   recon_voxel_add*(events, polarity) ...   recon_voxel_get / _get_device (any number of times)
 *     [recon_voxel_reset]   recon_voxel_end
 *   voxel_begin  needs an open reconstruction.  Copies the grids to the device as view_begin copies views, allocates
 *              n_grids * n_bins fp32 planes of Wv x Hv (and their 2^-30 fixed-point twins when CMX_OPT_DETERMINISTIC was 1 at
 *              recon_begin) and zeroes them and one vote counter per grid.  A second voxel_begin starts over.
 *              CMX_ERR_INVALID_ARG: every rule of view_begin (Wv or Hv outside [4, 8192]; a quaternion that is zero or not finite;
 *              fx or fy not finite or <= 0; cx or cy not finite; t_lo_ns >= t_hi_ns); n_bins outside [1, 64]; n_grids * n_bins
 *              outside [1, 4096]; n_grids * n_bins * Wv * Hv > 2^28; t_hi_ns - t_lo_ns above 2^53 (the difference is formed without
 *              signed overflow).  The bin axis needs a FINITE span -- beyond 2^53 ns the fp64 image of t - t_lo is not exact -- so a
 *              range that stands for all time (trajectory.ALL_TIME_NS, crop_view's default) is refused here although view_begin
 *              takes it.  Ranges may overlap, nest or leave gaps.
 *   voxel_add* ONE call = the vote loop of add* over exactly the events handed in -- the same batches, batch times and batch poses,
 *              sampling restarting at every batch start, the lone trailing event skipped, the same validation and status codes,
 *              complete before the first vote: a call that fails validation adds nothing.  Per sampled event i, in fp64 unless
 *              stated otherwise:
 *                  ray_w = R_batch * bearing                      (the vote kernels' own function, the pose at the BATCH time)
 *                  for every grid with t_lo_ns <= t_i < t_hi_ns   (t_i the event's OWN timestamp, compared as integers):
 *                      projection, vote test, cell (xx, yy) and fp32 dx, dy exactly as in view_add* above
 *                      n_bins >= 2:  scale = (double)(n_bins - 1) / (double)(t_hi_ns - t_lo_ns)   (formed once, on the host)
 *                                    tau = (double)(t_i - t_lo_ns) * scale,   b0 = min((int)tau, n_bins - 2),   f = (float)(tau - b0)
 *                                    bin b0 gets wt = 1.f - f, bin b0 + 1 gets wt = f
 *                      n_bins == 1:  the one bin gets wt = 1.f
 *                      each of the four cells of such a bin receives  s * (wt * wb)  in fp32, wb the fp32 bilinear product of add*
 *                      ((1-dx)(1-dy), dx(1-dy), (1-dx)dy, dx dy);  s = +1 always when signed_polarity == 0 (polarity is then
 *                      neither needed nor read), otherwise +1 for polarity != 0 and -1 for any other value
 *                      one count for the grid: an event counts once, not once per bin
 *              Deterministic mode: each magnitude is converted, to_fix(wt * wb), negated as an integer for s = -1 and added as a
 *              64-bit integer into the fixed-point twin; the cells are two's complement and are read as SIGNED.  A bin whose wt is
 *              zero may be skipped: that changes no sum.
 *              Polarity: pol[i] (one byte per event; NULL is allowed only when signed_polarity == 0), the byte at off_polarity of
 *              record i (not looked at for an unsigned set), or the store's own.
 *   voxel_get  out[g][b][yy][xx] fp32, contiguous: count * n_bins planes of Wv x Hv for grids [first_grid, first_grid + count), or
 *              NULL; n_voted = count counters or NULL.  CMX_ERR_INVALID_ARG when the range leaves the set.  Accumulation may continue.
 *   voxel_get_device  the same planes into a device pointer on the context's device (e.g. a torch tensor): nothing crosses the host.
 *              Runs on the context's stream and returns when d_out is complete.
 *   voxel_reset  clears the planes and the counters and keeps the grids.   voxel_end frees the set (without a set: CMX_OK).
 *   state      as for the views: the calls read the knots the reconstruction holds NOW and nothing else of it, and write only the
 *              grid planes and their counters.  recon_begin and recon_end free the set; restart and voxel_reset clear it; EVERY
 *              other call leaves it alone.  A view set and a voxel set may be open at the same time.
 *   status     CMX_ERR_STATE before recon_begin, before voxel_begin (add*, get*, reset), on a group handle, and for add_from on a
 *              store without polarity when the set is signed; CMX_ERR_INVALID_ARG for pol == NULL with a signed set.
 * Deterministic mode: every cell is a sum of integers -- bitwise identical from run to run, for any slicing at batch multiples,
 * through the three ingest paths, and whatever other grids are in the set.  Otherwise votes are fp32 atomics. */
int cmx_backend_recon_voxel_begin(cmx_ctx *ctx, int Wv, int Hv, int n_bins, int signed_polarity, int n_grids, const cmx_recon_view *grids);
int cmx_backend_recon_voxel_add(cmx_ctx *ctx, int64_t n, const uint16_t *x, const uint16_t *y, const int64_t *t_ns,
                                const uint8_t *pol /* n bytes; may be NULL only when signed_polarity == 0 */);
int cmx_backend_recon_voxel_add_aos(cmx_ctx *ctx, int64_t n, const void *events, const cmx_aos_layout *layout, size_t off_polarity);
int cmx_backend_recon_voxel_add_from(cmx_ctx *ctx, const cmx_events *ev, int64_t first, int64_t count);
int cmx_backend_recon_voxel_get(cmx_ctx *ctx, int first_grid, int count, float *out /* count*n_bins*Hv*Wv or NULL */,
                                int64_t *n_voted /* count or NULL */);
int cmx_backend_recon_voxel_get_device(cmx_ctx *ctx, int first_grid, int count, float *d_out /* device pointer on the context's device */);
int cmx_backend_recon_voxel_reset(cmx_ctx *ctx);
int cmx_backend_recon_voxel_end(cmx_ctx *ctx);
/* Time surfaces (surfaces of active events), motion-compensated: for every pixel the timestamp of the most recent event that landed
 * there, per polarity -- what corner detectors, HATS / TORE-style descriptors and network front ends read, usually through an
 * exponential decay.  A set of S surfaces is attached to an open reconstruction; a surface is a cmx_recon_view -- orientation,
 * intrinsics, [t_lo_ns, t_hi_ns) -- and trajectory.frame_views' and crop_view's output can be passed as it is.
 *     recon_surface_begin(surfaces)   recon_surface_add*(events, polarity) ...   recon_surface_get / _get_device / _decay /
 *     _decay_device (any number of times)   [recon_surface_reset]   recon_surface_end
 *   layout     C = by_polarity ? 2 : 1 channels; cells[s][c][yy][xx], contiguous.  Channel 0 is ON (polarity != 0), channel 1 is
 *              OFF -- the order of pol_get's arguments.  With by_polarity == 0 there is one channel and polarity is neither needed
 *              nor read.
 *   surface_begin  needs an open reconstruction.  Validates everything, then allocates all or nothing: the surfaces on the device as
 *              view_begin copies views, n_surfaces * C planes of Wv x Hv int64 cells, every one set to INT64_MIN ("no event"), and
 *              one vote counter per surface.  A second surface_begin starts over.
 *              CMX_ERR_INVALID_ARG: every rule of view_begin (Wv or Hv outside [4, 8192]; a quaternion that is zero or not finite;
 *              fx or fy not finite or <= 0; cx or cy not finite; t_lo_ns >= t_hi_ns); n_surfaces outside [1, 4096];
 *              n_surfaces * C * Wv * Hv > 2^28 (cells of 8 bytes: 2 GB, the footprint of a view set's fixed-point twins);
 *              t_lo_ns == INT64_MIN (the empty marker can then never be a vote).  A range that stands for all time
 *              (trajectory.ALL_TIME_NS, crop_view's default) is ACCEPTED, as view_begin accepts it and voxel_begin does not: a
 *              surface has no bin axis.  Ranges may overlap, nest or leave gaps.
 *   surface_add*  ONE call = the vote loop of add* over exactly the events handed in -- the same batches, batch times and batch
 *              poses, sampling restarting at every batch start, the lone trailing event skipped, the same validation and status
 *              codes, complete before the first vote: a call that fails validation adds nothing.  Per sampled event i, in fp64:
 *                  ray_w = R_batch * bearing                        (the vote kernels' own function, the pose at the BATCH time)
 *                  for every surface with t_lo_ns <= t_i < t_hi_ns  (t_i the event's OWN timestamp, compared as integers -- the
 *                                                                    voxel rule):
 *                      projection and vote test exactly as in view_add* above  (v.z > 0 && 1 <= u < Wv-2 && 1 <= w < Hv-2, in
 *                          floating point before any conversion)
 *                      cx = (int)(u + 0.5),  cy = (int)(w + 0.5)    (the NEAREST pixel; inside the plane because of the test)
 *                      c  = by_polarity && polarity == 0 ? 1 : 0
 *                      cells[s][c][cy][cx] = max(cells[s][c][cy][cx], t_i)   as a signed 64-bit integer
 *                      one count for the surface
 *              Polarity: pol[i] (one byte per event; NULL is allowed only when by_polarity == 0), the byte at off_polarity of record
 *              i (not looked at for a merged set), or the store's own.
 *   surface_get  cells = count * C planes of Wv x Hv int64 for surfaces [first, first + count), or NULL: absolute nanoseconds, and
 *              INT64_MIN in a cell no event reached; n_voted = count counters (events: one per event and surface) or NULL.
 *              CMX_ERR_INVALID_ARG when the range leaves the set.  Accumulation may continue.
 *   surface_get_device  the same cells into a device pointer on the context's device (e.g. a torch int64 tensor): nothing crosses the
 *              host.  Runs on the context's stream and returns when d_cells is complete.
 *   surface_decay / _decay_device  one device pass writes fp32 in the layout above, to the host (staged through device memory of the
 *              set's own) or to a device pointer on the context's device.  With t_ref of surface s = t_ref_ns[s - first], or that
 *              surface's t_hi_ns when t_ref_ns is NULL (a host array in both forms), and T the cell:
 *                  T == INT64_MIN   ->  0.0f
 *                  T >= t_ref       ->  1.0f
 *                  otherwise        ->  (float)exp(-((double)(uint64_t)(t_ref - T) / tau_ns))
 *              the difference formed without signed overflow, quotient and exp in fp64, rounded once.  Results below FLT_MIN may be
 *              flushed to zero or left denormal.  CMX_ERR_INVALID_ARG: tau_ns not finite or <= 0; a range outside the set; a null
 *              output with count > 0.  The cells stay as they are.
 *   surface_reset  sets every cell back to INT64_MIN and the counters to zero and keeps the surfaces.   surface_end frees the set
 *              (without a set: CMX_OK).
 *   state      as for the views and the voxel grids: the calls read the knots the reconstruction holds NOW and nothing else of it,
 *              and write only the surface cells and their counters.  recon_begin and recon_end free the set; restart and
 *              surface_reset clear it to empty; EVERY other call leaves it alone.  A view set, a voxel set and a surface set may be
 *              open together.  The calls work with a gradient pass open, with events bound, after freeze_head and after
 *              release_head.
 *   status     CMX_ERR_STATE before recon_begin, before surface_begin (add*, get*, decay*, reset), on a group handle, and for
 *              add_from on a store without polarity when the set is by polarity; CMX_ERR_INVALID_ARG for pol == NULL with a
 *              by-polarity set and for off_polarity outside the record.
 * Reproducibility: a cell is a maximum of integers, which commutes and is idempotent -- bitwise identical from run to run, through
 * the three ingest paths, for any slicing at batch multiples, for the calls of a split IN ANY ORDER, and whatever other surfaces are
 * in the set, with CMX_OPT_DETERMINISTIC 0 or 1: the option changes nothing here and there is no fixed-point twin. */
int cmx_backend_recon_surface_begin(cmx_ctx *ctx, int Wv, int Hv, int by_polarity, int n_surfaces, const cmx_recon_view *surfaces);
int cmx_backend_recon_surface_add(cmx_ctx *ctx, int64_t n, const uint16_t *x, const uint16_t *y, const int64_t *t_ns,
                                  const uint8_t *pol /* n bytes; may be NULL only when by_polarity == 0 */);
int cmx_backend_recon_surface_add_aos(cmx_ctx *ctx, int64_t n, const void *events, const cmx_aos_layout *layout, size_t off_polarity);
int cmx_backend_recon_surface_add_from(cmx_ctx *ctx, const cmx_events *ev, int64_t first, int64_t count);
int cmx_backend_recon_surface_get(cmx_ctx *ctx, int first, int count, int64_t *cells /* count*C*Hv*Wv or NULL */,
                                  int64_t *n_voted /* count or NULL */);
int cmx_backend_recon_surface_get_device(cmx_ctx *ctx, int first, int count, int64_t *d_cells /* device pointer on the context's device */);
int cmx_backend_recon_surface_decay(cmx_ctx *ctx, int first, int count, const int64_t *t_ref_ns /* count, or NULL */, double tau_ns,
                                    float *out /* count*C*Hv*Wv */);
int cmx_backend_recon_surface_decay_device(cmx_ctx *ctx, int first, int count, const int64_t *t_ref_ns /* host: count, or NULL */,
                                           double tau_ns, float *d_out /* device pointer on the context's device */);
int cmx_backend_recon_surface_reset(cmx_ctx *ctx);
int cmx_backend_recon_surface_end(cmx_ctx *ctx);
/* Whole-trajectory contrast and its gradient with respect to a LEFT increment of every control pose, on top of an open
 * reconstruction -- the evaluation one bundle adjustment over the whole recording needs, for a spline of any knot count:
 *     recon_begin   recon_add*(events) ...   recon_contrast(want_grad)   recon_grad_add*(the same events) ...   recon_grad_get
 * With the plane holding one vote loop over events E along knots q, contrast is the contrast of GaussianBlur(plane, blur_sigma) and
 * grad[3k + c] what the back end's global_contrast_fdf returns for num_fixed = 0, zero increments, an all-zero map (alpha = 0) and
 * every event on one side of the old / new split: cmx_backend_set_window(num_fixed = 0, IG = NULL) + cmx_backend_eval(0), without
 * the 64-knot limit.  contrast_measure: CMX_VARIANCE, CMX_MEAN_SQUARE, anything else = variance; N = Wp * Hp.  The gradient is
 * formed the adjoint way: Jt = G^T (G plane), per event the two directional differences of Jt at its vote cell times
 * d(pixel)/d(rotation), summed per batch, through the batch's 3 x 3N spline Jacobian onto the N knots it touches;
 * grad = (2/N)(S1 - mu S2) with the border term S2 accumulated apart.
 *   restart    new knot values (K x 4, xyzw) for the spline description, batch size, sample rate and deterministic setting of begin;
 *              zeroes the plane, both counters and any gradient state; allocates and frees nothing (once per trial point).
 *   contrast   the image pass over the plane as accumulated so far; never changes the plane (add* may follow).  Every panorama size
 *              and every blur_sigma cmx_backend_set_window accepts (CMX_ERR_INVALID_ARG beyond radius 12).  want_grad != 0: Jt stays
 *              resident, the gradient sums are zeroed and a gradient pass is OPEN; CMX_ERR_INVALID_ARG when Wp <= 2r+1 or Hp <= 2r+1
 *              (r = blur radius: the folded G^T needs single reflections; there is no derivative-plane fallback for 3K planes).
 *              Taps, G^T 1 factors, Jt and the moment rows belong to the reconstruction: the window's blur state and image buffers
 *              are not touched.  A cost-only call leaves an open pass open unless it changes blur_sigma.
 *   grad_add*  the SECOND pass over the same events, in the same calls and cuts as the add* calls (batches start at each call's
 *              first event).  Validation and status codes of add*; a call that fails validation adds nothing.  Same internal slices
 *              and staging.  CMX_ERR_STATE without an open pass; begin, restart and every add* close it.
 *   grad_get   grad = 3K doubles.  CMX_ERR_STATE unless the pass's sampled count and voted count both equal the plane's n_sampled /
 *              n_inside (other events or other cuts were fed).  May be called repeatedly.
 *   eval_from  restart (knots_xyzw != NULL) + add_from + contrast + (grad != NULL: grad_add_from + grad_get) in one call.
 *   end        also frees Jt, the image-pass scratch and the 2 x 3K gradient sums (allocated at the first want_grad).
 * All of them return CMX_ERR_STATE before begin and on a group handle.
 * CMX_OPT_DETERMINISTIC = 1 at begin: contrast and gradient are bitwise identical from run to run for the same sequence of calls
 * (every floating-point sum has a fixed order; a workgroup whose 2048 events span more than 262 knot intervals -- a gap in the
 * recording -- adds its out-of-window batches with atomics) and agree across slicings to summation order. */
int cmx_backend_recon_restart(cmx_ctx *ctx, const double *knots_xyzw);
int cmx_backend_recon_contrast(cmx_ctx *ctx, double blur_sigma, int contrast_measure, int want_grad, double *contrast);
int cmx_backend_recon_grad_add(cmx_ctx *ctx, int64_t n, const uint16_t *x, const uint16_t *y, const int64_t *t_ns);
int cmx_backend_recon_grad_add_aos(cmx_ctx *ctx, int64_t n, const void *events, const cmx_aos_layout *layout);
int cmx_backend_recon_grad_add_from(cmx_ctx *ctx, const cmx_events *ev, int64_t first, int64_t count);
int cmx_backend_recon_grad_get(cmx_ctx *ctx, double *grad /* 3K */);
int cmx_backend_recon_eval_from(cmx_ctx *ctx, const cmx_events *ev, int64_t first, int64_t count,
                                const double *knots_xyzw /* K x 4, or NULL = keep */, double blur_sigma,
                                int contrast_measure, double *contrast, double *grad /* 3K or NULL */);
/* Bound events: an optimiser over the whole trajectory evaluates the SAME events hundreds of times along slightly moved knots.
 * eval_from reads the event store again every time and votes with one global atomic per bilinear corner; these calls hand the
 * events over once and vote through LDS:
 *     recon_begin   recon_bind_from(events)   recon_eval_bound(knots) ...   recon_unbind / recon_end
 *   bind_from   validation and status codes of add_from, all of it before any device state changes.  Copies what the evaluations
 *               need into memory the reconstruction owns -- the events of the range the sampling selects, packed in time order, and
 *               the batch pose times -- so the store may be pushed to, compacted or closed afterwards.  Votes nothing; the plane, the
 *               counters and the knots stay as they are; an open gradient pass is closed.  A second bind replaces the first; a call
 *               that fails validation leaves an earlier binding intact.  count of 0 or 1 is valid and binds nothing to vote.
 *               Limit: at most 2^30 sampled events (CMX_ERR_INVALID_ARG above: sorted positions are 32-bit).  Resident memory: 16
 *               bytes per sampled event and 80 per batch, plus the sort's tables (a function of the panorama: 34 MB at 4096 x 2048).
 *   unbind      frees the bound buffers; CMX_OK without a binding.  begin and end drop a binding too; restart keeps it.
 *   eval_bound  by definition restart(knots_xyzw, or the current knots when NULL) followed by eval_from over the bound events: it
 *               always starts from a zeroed plane, and leaves the reconstruction as eval_from would -- the plane readable by get /
 *               render, n_sampled and n_inside exact, the gradient repeatable by grad_get, later add* calls accumulating on top.
 *               blur_sigma, contrast_measure and the size rule of grad != NULL as in contrast.  CMX_ERR_STATE without a binding.
 *               How: a batch-pose table (72 bytes per batch) behind the knots' logarithms; the bound events sorted by the 32 x 32
 *               destination tile of their vote -- in front of the first evaluation after a bind, and again in front of an evaluation
 *               when more than 3 % of the previous one's voting events left their LDS window (the rule of the window path); one
 *               workgroup per chunk of a tile's events votes into a 64 x 64 window of 64-bit 2^-30 fixed-point cells in LDS and
 *               adds every touched cell to the plane once; a vote outside the window goes to the plane directly, so the result is
 *               exact wherever the knots move.  The sort, the chunk table and the counters belong to the reconstruction: the
 *               window's sort and cmx_get_stats' re-sort count are not touched.  The gradient pass runs over the time-ordered copy
 *               in eval_from's slices.  Under cmx_timing_enable: CMX_T_POSE = the pose table, CMX_T_SPLAT = the vote kernel,
 *               CMX_T_BATCH = the tile sort (bracketed on the stream), when one ran.
 *   bound_info  any pointer may be NULL; all zero without a binding.  *n_events = events bound, *n_sampled = those the sampling
 *               selects, *sorts = tile sorts run since the bind, *fallback_frac = the share of the last evaluation's voting events
 *               that left their LDS window.
 * CMX_OPT_DETERMINISTIC = 1 at begin: plane, counters and contrast are bitwise those of eval_from over the same events at the same
 * knots (the same integers are added, in another order); the gradient is bitwise identical from run to run and agrees with
 * eval_from's to summation order.  Otherwise every window's sum is rounded to fp32 once, when it is added to the plane. */
int cmx_backend_recon_bind_from(cmx_ctx *ctx, const cmx_events *ev, int64_t first, int64_t count);
int cmx_backend_recon_unbind(cmx_ctx *ctx);
int cmx_backend_recon_eval_bound(cmx_ctx *ctx, const double *knots_xyzw /* K x 4, or NULL = keep */, double blur_sigma,
                                 int contrast_measure, double *contrast, double *grad /* 3K or NULL */);
int cmx_backend_recon_bound_info(cmx_ctx *ctx, int64_t *n_events, int64_t *n_sampled, int64_t *sorts, double *fallback_frac);
/* A frozen head, and the whole bundle adjustment as one call.  Online, the recording grows, the head of the trajectory is settled
 * and only its tail -- of any knot count -- is free.  An event batch whose pose reads fixed knots alone votes the same cells at every
 * trial point: with s the knot segment of its pose time it is FROZEN when s + order - 1 < num_fixed, and since batch times do not
 * decrease the frozen batches are a prefix of the binding's.
 *     recon_begin   recon_bind_from(events)   [recon_freeze_head(num_fixed)]   recon_eval_bound(knots) ... | recon_solve(...)
 *   freeze_head   needs a binding (CMX_ERR_STATE) and 0 <= num_fixed < K (CMX_ERR_INVALID_ARG).  Votes the frozen batches ONCE, at the
 *                 knots the reconstruction holds (those of begin, restart or the last evaluation), into a base plane of the
 *                 reconstruction's own -- fp32, or the 2^-30 fixed-point plane under CMX_OPT_DETERMINISTIC -- and records how many of
 *                 their events voted.  The plane, its counters and the knots stay as they are; an open gradient pass is closed.
 *                 num_fixed = 0 removes the frozen head and frees the base.  A second call replaces the first.
 *   dropped by    begin, end, bind_from, unbind and restart (so also by eval_from with knots); kept by eval_bound.
 *   eval_bound    with a frozen head: knots_xyzw (when given) must carry the first num_fixed quaternions bytewise as they were at the
 *                 freeze, CMX_ERR_INVALID_ARG otherwise and nothing changes.  The plane starts from the base; the pose table, the tile
 *                 sort (of the active events alone, with a chunk table at the chunk rule of their count, re-sorted by the 3 % rule on
 *                 THEIR votes), the LDS vote pass and the gather pass run over the active batches only.  What it leaves is what
 *                 eval_bound leaves without one: the full plane for get / render, exact n_sampled / n_inside (base plus active), a
 *                 gradient grad_get repeats -- grad[0 .. 3 num_fixed) is zero by definition, the other entries are the full
 *                 gradient's (frozen batches reach no free knot; Jt is built from the full plane).  grad_get's test reads base plus
 *                 active counts against the plane's.  Deterministic mode: plane, counters and contrast bitwise those of the unfrozen
 *                 evaluation; the free gradient to summation order (the gather's runs start at the first active batch), and bitwise
 *                 when no batch is frozen.
 *   frozen_info   any pointer may be NULL; all zero without a frozen head.  *frozen_batches = b_act, the number of frozen batches,
 *                 *frozen_sampled = the sampled events in them.
 *   solve         FR-CG (the machine of cmx_backend_solve / cmx_frcg_minimize) over a left increment of every control pose but the
 *                 first num_fixed, cost = -contrast of the bound events' panorama; constants as in cmx_frcg_minimize.  Per trial point
 *                 the start knots are moved by cmx_traj_incremental_update's own code on the host, uploaded from pinned staging, and
 *                 evaluated by eval_bound's sequence of launches with ONE host wait at the end; with a gradient the device forms
 *                 (2/N)(S1 - mu S2) for the free parameters and writes them to host memory (no read-back of the 2 x 3K sums).
 *                 freeze_head != 0: freezes at the start knots, solves, and leaves the frozen head in place; 0: any frozen head is
 *                 removed and every event is evaluated every time.  Errors before anything changes: CMX_ERR_STATE without a binding;
 *                 CMX_ERR_INVALID_ARG for num_fixed outside [0, K), a panorama too small for the adjoint gradient at blur_sigma, or a
 *                 non-finite constant.  On return knots_xyzw holds the refined knots and the reconstruction their evaluation -- plane,
 *                 counters, contrast -- at the price of one more cost-only evaluation only if the last trial point was another one;
 *                 report as filled by cmx_backend_solve (n_f / n_df do not count that one). */
int cmx_backend_recon_freeze_head(cmx_ctx *ctx, int num_fixed);
int cmx_backend_recon_frozen_info(cmx_ctx *ctx, int *num_fixed, int64_t *frozen_batches, int64_t *frozen_sampled);
/* (cmx_backend_recon_solve is declared with the other solves, below cmx_solve_report) */
/* A binding that grows: the recording gets longer, the spline with it, the freeze line moves forward and the settled events'
 * memory is given back.  Per step of an online host:
 *     recon_extend(K_new, knots)   recon_bind_append_from(new events)   recon_solve(CMX_RECON_KEEP_HEAD) | recon_eval_bound ...
 *     recon_advance_head(num_fixed_new)   recon_release_head()
 * All of them: a plain back-end context with a reconstruction begun (CMX_ERR_STATE on NULL, on a group handle, before begin), and
 * complete validation before any device state changes -- a call that fails validation leaves the reconstruction as it was.
 *   extend         restart that may lengthen the spline and keeps a frozen head.  K_new >= K (CMX_ERR_INVALID_ARG below, and above
 *                  begin's limit); order, start_ns, dt_ns, batch size, sample rate and the deterministic setting stay those of begin.
 *                  Replaces the knots, zeroes the plane, both counters and the gradient state, closes an open gradient pass, keeps
 *                  the binding.  With a frozen head the first num_fixed quaternions must be bytewise those of the freeze
 *                  (CMX_ERR_INVALID_ARG otherwise).  With K_new == K and no frozen head it is restart.
 *   bind_append_from  needs a binding (CMX_ERR_STATE).  Afterwards the binding is exactly what bind_from over the concatenation of
 *                  all ranges bound so far would hold: batch cuts, batch pose times, the sampled events in packed order, bound_info's
 *                  counts.  Validation and status codes of bind_from, plus: the first new event may not be earlier than the last
 *                  bound one (CMX_ERR_TIME_ORDER); CMX_ERR_SPLINE_RANGE is judged against the K of this moment, so an online
 *                  caller extends first.  Reads only [first, first + count) of the store: events bound earlier may have been dropped
 *                  from it.  The last batch of a binding may be open -- fewer than event_batch_size events, or a lone trailing event
 *                  no batch has opened -- and an append cuts it again: its pose time moves with its new last event, the sampling
 *                  stride continues from its start.  The binding keeps the raw events of that open tail (at most
 *                  event_batch_size of them) for this.  Work is proportional to count + event_batch_size; buffers grow
 *                  geometrically; a failed allocation leaves the binding as it was.  A frozen head is kept; when the batch to be cut
 *                  again is itself frozen: CMX_ERR_STATE, nothing changes.  (New batches behind a head that had frozen EVERY batch
 *                  are evaluated as active ones until advance_head looks at them: exact, but the deterministic gradient then agrees
 *                  with a fresh freeze's to summation order only.)  The limit of 2^30 sampled events applies to the RESIDENT ones
 *                  (see release_head).  count == 0 is valid and changes nothing but closing an open gradient pass.
 *   advance_head   needs a binding (CMX_ERR_STATE) and num_fixed <= num_fixed_new < K (CMX_ERR_INVALID_ARG; going back is
 *                  freeze_head's job); without a frozen head it is freeze_head(num_fixed_new).  At the knots the reconstruction
 *                  holds, the batches the prefix rule newly names are voted ONCE into the existing base, on top of what is there,
 *                  and their voting count is added to the base's; the base is neither cleared nor voted again.  It may freeze nothing
 *                  new.  Deterministic mode: base, counters and every later evaluation are bitwise those of a fresh bind_from over
 *                  everything + freeze_head(num_fixed_new) at the same knots; default mode: equal to summation order.
 *   release_head   needs a binding (CMX_ERR_STATE).  Frees the resident memory of the frozen batches' events (their packed events,
 *                  batch times and pose-table rows).  The released entries are dead space until there is more of it than live entries, or
 *                  an append runs out of room; then the active tail moves into buffers of twice its size and the old ones are freed,
 *                  so the capacity stays within a small constant factor of the largest active tail, whatever the recording's length.
 *                  Evaluations are unchanged -- plane, counters, contrast, and the gradient bitwise in deterministic mode;
 *                  bound_info keeps reporting the totals since the bind.  Nothing to release (no frozen head, nothing newly
 *                  frozen) is valid.  Once events are released their votes live in the base alone, so restart, eval_from with knots,
 *                  freeze_head (any argument) and recon_solve with freeze_head 0 or 1 return CMX_ERR_STATE and change nothing;
 *                  begin, end, bind_from and unbind work and drop everything.
 *   online_info    any pointer may be NULL; all zero without a binding.  Batches, events and sampled events released so far, and the
 *                  sampled events resident now.
 *   solve          freeze_head == CMX_RECON_KEEP_HEAD: the solve runs under the frozen head as it stands.  CMX_ERR_STATE without
 *                  one; CMX_ERR_INVALID_ARG unless num_fixed equals the head's and the start knots carry the head's bytes.  In
 *                  deterministic mode it returns the knots of a solve with freeze_head = 1 over a fresh binding of the same events
 *                  from the same start, byte for byte. */
#define CMX_RECON_KEEP_HEAD 2
int cmx_backend_recon_extend(cmx_ctx *ctx, int K_new, const double *knots_xyzw /* K_new x 4 */);
int cmx_backend_recon_bind_append_from(cmx_ctx *ctx, const cmx_events *ev, int64_t first, int64_t count);
int cmx_backend_recon_advance_head(cmx_ctx *ctx, int num_fixed_new);
int cmx_backend_recon_release_head(cmx_ctx *ctx);
int cmx_backend_recon_online_info(cmx_ctx *ctx, int64_t *released_batches, int64_t *released_events, int64_t *released_sampled,
                                  int64_t *resident_sampled);

/* ------------------------------------------------------------------ split-phase (multi-GPU) ------------
 * The IWE is a sum over events, the contrast a non-linear function of the SUMMED image, so ranks exchange
 * between splat and blur/reduce.  Each rank loads its contiguous range of event
 * batches with set_packet / set_window, then per evaluation:
 *     cmx_*_accumulate(ctx, x, want_grad)     zero + splat the rank's partial planes
 *     all-reduce(sum) cmx_accum_ptr(ctx) [cmx_accum_count floats]      (RCCL, caller-side)
 *     cmx_*_finish(ctx, &contrast, grad)      blur + reduce on the summed planes
 *   with CMX_GRAD_ADJOINT the planes are I only and finish() returns the rank's PARTIAL gradient
 *   (sum over its own events): all-reduce(sum) that small vector too.
 * cmx_set_accum_buffer lets the caller own the accumulation memory (e.g. a torch tensor, so
 * torch.distributed can all-reduce it in place); it must hold cmx_accum_capacity(ctx) floats. */
size_t cmx_accum_capacity(const cmx_ctx *ctx);             /* floats needed for the worst case of this context */
int cmx_set_accum_buffer(cmx_ctx *ctx, void *device_ptr, size_t n_floats);
void *cmx_accum_ptr(const cmx_ctx *ctx);                   /* device pointer of the accumulation planes */
size_t cmx_accum_count(const cmx_ctx *ctx);                /* floats written by the last accumulate() */
int cmx_frontend_accumulate(cmx_ctx *ctx, const double omega[3], int want_grad);
int cmx_frontend_finish(cmx_ctx *ctx, double *contrast, double *grad);
int cmx_backend_accumulate(cmx_ctx *ctx, const double *drotv, int want_grad);
int cmx_backend_finish(cmx_ctx *ctx, double *contrast, double *grad);
/* With CMX_GRAD_ADJOINT the gradient needs a second, tiny exchange (each rank gathers over its own events from the
 * common Itilde plane).  finish() = finish_begin() + finish_end(); between the two the rank's partial gradient sums
 * sit in device memory at cmx_grad_ptr(ctx) [cmx_grad_count(ctx) doubles] for an in-place all-reduce(sum); nothing
 * is synchronised with the host until finish_end().  cmx_set_grad_buffer makes that buffer caller-owned. */
int cmx_frontend_finish_begin(cmx_ctx *ctx, int want_grad);
int cmx_frontend_finish_end(cmx_ctx *ctx, double *contrast, double *grad);
int cmx_backend_finish_begin(cmx_ctx *ctx, int want_grad);
int cmx_backend_finish_end(cmx_ctx *ctx, double *contrast, double *grad);
void *cmx_grad_ptr(const cmx_ctx *ctx);
size_t cmx_grad_count(const cmx_ctx *ctx);
int cmx_set_grad_buffer(cmx_ctx *ctx, void *device_ptr, size_t n_doubles);

/* Native exchange: attach an RCCL communicator to the context (one process per GPU) and every cmx_*_eval / cmx_*_solve
 * performs the all-reduces itself, in place, on the context's stream -- partial planes after the splat, and the 2P
 * partial gradient sums after the gather pass (adjoint mode).  All ranks therefore see identical contrast / gradient
 * and take identical optimiser decisions.  Every rank must use the same options (cmx_set_option) and issue the same
 * sequence of calls; which collectives an evaluation issues then depends on rank-invariant state only (plane size,
 * options, call sequence) -- never on how many events a rank happens to hold (an empty shard takes part like any other).
 * Back-end planes of 1 MB and more are exchanged as a SET OF TILES (64 x 16 pixels): the tiles exchanged -- packed from both
 * planes into one staging buffer with the tile-occupancy map behind them, one collective -- are those any rank flagged in
 * the PREVIOUS evaluation, dilated by one tile in every direction (the whole planes on a window's first evaluation, or when
 * the set exceeds half of the map) -- no host synchronisation between splat and blur.  A kernel lists the flagged tiles the set
 * did not cover; if there are any (parameters jumped) the evaluation is completed by exchanging exactly those and finishing again.
 * Smaller planes travel whole.  cmx_get_stats reports host synchronisations inside sharded evaluations (0), misses and set size.
 * Rank 0 creates the 128-byte id (cmx_comm_unique_id); the launcher distributes it by whatever means it has
 * (torch.distributed broadcast in bench.py, MPI, a file).  RCCL is dlopen()ed at this point only; hosts that never
 * attach a communicator do not need it installed. */
#define CMX_COMM_ID_BYTES 128
int cmx_comm_unique_id(char id[CMX_COMM_ID_BYTES]);
int cmx_comm_attach(cmx_ctx *ctx, const char id[CMX_COMM_ID_BYTES], int rank, int nranks);
int cmx_comm_detach(cmx_ctx *ctx);
/* The same exchange points over a caller-supplied transport (MPI, a shared-memory ring, a test harness): `fn` must
 * all-reduce `count` elements at `device_buf` IN PLACE across the nranks participants, ordered after the work already
 * queued on `hip_stream` and before work queued afterwards (i.e. enqueue on that stream, or synchronise it, exchange, and
 * return), and return 0 on success.  Ranks call it in the same order with the same count / dtype / op. */
enum { CMX_DT_U8 = 0, CMX_DT_F32 = 1, CMX_DT_F64 = 2 };
enum { CMX_OP_SUM = 0, CMX_OP_MAX = 1 };
typedef int (*cmx_allreduce_fn)(void *user, void *device_buf, size_t count, int dtype, int op, void *hip_stream);
int cmx_comm_attach_custom(cmx_ctx *ctx, cmx_allreduce_fn fn, void *user, int rank, int nranks);
/* What is attached, AS THE COMMUNICATOR ITSELF REPORTS IT: *transport = 0 none, 1 RCCL (rank / nranks from ncclCommUserRank /
 * ncclCommCount of the live communicator -- not the numbers passed at attach), 2 caller-supplied or a group's direct transport
 * (the numbers given at attach).  On a group handle: member 0's communicator.  Any pointer may be NULL. */
int cmx_comm_info(cmx_ctx *ctx, int *rank, int *nranks, int *transport);

/* ------------------------------------------------------------------ one-process multi-GPU: a GROUP ---------
 * The reference's host is ONE process with ONE back-end thread and ONE GSL instance (src/cmax_slam.cpp:92,
 * src/backend/global_optim_contrast_gsl.cpp:23-33): it cannot be started once per GPU.  cmx_backend_create_group returns an
 * ordinary back-end handle whose evaluations fan out to n_devices member contexts: cmx_backend_set_window shards the window
 * by whole event batches (member r = rank r of the one-process-per-GPU form; event_pano_warper.cpp:188-196 is the loop being
 * split), cmx_backend_eval / cmx_backend_solve run the members' splat, the plane / tile-set exchange, blur and gather on all
 * devices, add the members' gradients on the calling thread (the gradient is linear in the members' row sums: no second
 * collective) and return ONE contrast / gradient -- the bodies of global_contrast_{f,df,fdf} do not
 * change, there is one optimiser and no launcher.  The map upkeep calls, cmx_set_option and cmx_destroy act on every member
 * (each keeps its own replica of IG); cmx_backend_get_plane / get_alpha / get_map / render_map / cmx_get_stats read member 0.  The caller
 * stays single-threaded; the group owns one worker thread per further member (queueing eight devices' launches from one
 * thread would take longer than the evaluation runs).  Not available on a group: the split-phase interface, caller-owned
 * buffers / streams, cmx_comm_attach*, cmx_backend_eval_many.  cmx_backend_set_window_from works on a group when the store was
 * created with cmx_events_create_group over the same devices.
 *   transport: CMX_GROUP_RCCL  -- ncclCommInitAll, one communicator per member (devices must be distinct);
 *              CMX_GROUP_DIRECT -- peer-to-peer reduce-scatter + all-gather kernels over the members' own buffers, ordered by
 *                                  HIP events (needs peer access between the devices; the only form for members that share
 *                                  ONE device, which is how a single-GPU box exercises all of this);
 *              CMX_GROUP_AUTO   -- MEASURED: every transport the devices allow is set up (members sharing a device: DIRECT only;
 *                                  no peer access: RCCL only), a production-sized exchange is timed through each at creation and
 *                                  the faster one kept (cmx_group_transport_info reports the choice and both timings).
 * n_devices == 1 returns a plain context (no group, no overhead).  Results equal the single-context evaluation of the whole
 * window to summation order (the planes are sums of the members' partial planes). */
enum { CMX_GROUP_AUTO = 0, CMX_GROUP_RCCL = 1, CMX_GROUP_DIRECT = 2 };
int cmx_backend_create_group(cmx_ctx **out, const int *devices, int n_devices, int W, int H, const double *lut, int Wp, int Hp,
                             int transport);
/* what a handle is made of: members, their devices, the transport in use, packed events per member of the current window,
 * host microseconds of the last fan-out (command published -> all members returned).  Any pointer may be NULL. */
int cmx_group_info(cmx_ctx *ctx, int *n_members, int *devices, int max_devices, int *transport, int64_t *events_per_member,
                   double *last_fanout_us);
/* how the transport in use was picked: *chosen = CMX_GROUP_RCCL / _DIRECT; *measured = 1 when CMX_GROUP_AUTO timed the candidates at
 * creation (20 staged exchanges of a 1 MB message -- a production tile set -- through every transport the devices allow, each member
 * on its own thread as an evaluation issues them) and kept the faster; *us_direct / *us_rccl = microseconds per exchange (-1: that
 * transport could not be set up on these devices -- e.g. RCCL for members sharing one device -- or was not timed).  Any pointer may
 * be NULL; a plain context reports CMX_GROUP_AUTO, 0, -1, -1. */
int cmx_group_transport_info(cmx_ctx *ctx, int *chosen, int *measured, double *us_direct, double *us_rccl);

/* ------------------------------------------------------------------ optimiser driver (host C++) ----------
 * The reference runs GSL's Fletcher-Reeves conjugate gradient around the cost functors
 * (src/frontend/local_optim_contrast_gsl.cpp:74-233, src/backend/global_optim_contrast_gsl.cpp:15-145).  These
 * entry points restate those driver loops (same constants and stopping rules) over a restated conjugate_fr
 * (GSL itself is not vendored by the reference); a host that keeps GSL simply does not call them. */
typedef struct {
  int iterations;      /* gsl_multimin_fdfminimizer_iterate calls (line searches) */
  int status;          /* 0 = converged on an accepted step, -2 = iteration limit, 27 = no progress (GSL codes) */
  int n_f, n_df;       /* cost-only and cost+gradient evaluations performed */
  double initial_cost; /* -contrast at the start */
  double final_cost;   /* -contrast at the returned parameters */
} cmx_solve_report;
/* ang_vel: in = warm start (the reference keeps ang_vel_ between packets), out = estimate */
int cmx_frontend_solve(cmx_ctx *ctx, double ang_vel[3], cmx_solve_report *report);
/* drotv: in = start (the reference uses 0), out = optimal incremental rotation vectors, n_params = 3*(K-num_fixed) */
int cmx_backend_solve(cmx_ctx *ctx, int n_params, double *drotv, cmx_solve_report *report);
/* the bundle adjustment over the bound events of a whole-trajectory reconstruction (see cmx_backend_recon_freeze_head above) */
int cmx_backend_recon_solve(cmx_ctx *ctx, double *knots_xyzw /* K x 4, in: start, out: refined */, int num_fixed, int freeze_head,
                            double blur_sigma, int contrast_measure, double step_size, double tol, double epsabs_grad, double tolfun,
                            int max_iterations, cmx_solve_report *report);
/* the same driver loop over an arbitrary functor triple (the shape of gsl_multimin_function_fdf); lets a host or a
 * test run the identical optimiser over any other implementation of the cost */
typedef double (*cmx_f_fn)(const double *x, void *params);
typedef void (*cmx_df_fn)(const double *x, void *params, double *g);
typedef void (*cmx_fdf_fn)(const double *x, void *params, double *f, double *g);
int cmx_frcg_minimize(cmx_f_fn f, cmx_df_fn df, cmx_fdf_fn fdf, void *params, int n, double *x, double step_size,
                      double tol, double epsabs_grad, double tolfun, int max_iterations, cmx_solve_report *report);
/* the same with a fourth callback that receives, in front of every cost-only evaluation, the line search's acceptance test
 * (threshold, mode: see cmx_hint_next_df) -- a host that keeps its own f / df / fdf bodies forwards it to cmx_hint_next_df
 * and gets the gated gradient pass; hint == NULL is cmx_frcg_minimize */
typedef void (*cmx_hint_fn)(double threshold, int mode, void *params);
int cmx_frcg_minimize_hinted(cmx_f_fn f, cmx_df_fn df, cmx_fdf_fn fdf, cmx_hint_fn hint, void *params, int n, double *x,
                             double step_size, double tol, double epsabs_grad, double tolfun, int max_iterations,
                             cmx_solve_report *report);

/* ------------------------------------------------------------------ control-pose initialisation (host C++) ---
 * what the back-end thread does between two window solves to turn the front end's
 * angular velocities into the control poses the next window starts from, and the once-per-camera bearing table.
 * Pure host fp64 (tens of poses x a handful of control poses); no context, no device work.  Quaternions are
 * (x,y,z,w); stamps are int64 ns; sequences must be strictly increasing in time (the reference keeps them in
 * std::map keyed by stamp). */
/* PoseGraphOptimizer::integrateAngVel (src/backend/pose_graph_optimizer.cpp:191-222): trapezoidal integration of the
 * n stamped angular velocities onto (pose_t_ns, pose_quat), post-multiplied.  prev_*: ang_vel_prev_ (in/out).
 * out_*: room for n poses; *n_out = number written (stale stamps are skipped unless first_time_window). */
int cmx_integrate_ang_vel(int n, const int64_t *t_ns, const double *ang_vel /* 3n */, int64_t pose_t_ns,
                          const double pose_quat[4], int64_t *prev_t_ns, double prev_ang_vel[3], int first_time_window,
                          int64_t *out_t_ns, double *out_quat /* 4n */, int *n_out);
/* {Linear,Cubic}Trajectory::generateCtrlPoses' count (src/backend/trajectory.cpp:205-214 / :480-489):
 * round((t_end - t_beg).toSec() / dt_knots) + 1 (order 2) or + 3 (order 4); -1 on bad arguments */
int cmx_num_ctrl_poses(int order, int64_t t_beg_ns, int64_t t_end_ns, double dt_knots);
/* {Linear,Cubic}Trajectory::fitCtrlPoses (src/backend/trajectory.cpp:112-192 / :357-464): least-squares B-spline
 * fit in the tangent space at the first pose, solved like Eigen's fullPivHouseholderQr().solve (zero free variables
 * when rank-deficient).  CMX_ERR_INVALID_ARG where the reference's CHECK_GE / Eigen index assertion would abort. */
int cmx_fit_ctrl_poses(int order, int n_poses, const int64_t *t_ns, const double *quat /* 4 n_poses */,
                       double t_beg_sec, double dt_knots, int num_cps, double *out_quat /* 4 num_cps */);
/* {Linear,Cubic}Trajectory::incrementalUpdate (src/backend/trajectory.cpp:221-238 / :491-499):
 * knot_i <- exp(drotv_{i-idx_beg}) * knot_i for i >= idx_beg; n_params = 3*(K-idx_beg) (what cmx_backend_solve returns) */
int cmx_traj_incremental_update(int K, double *knots /* 4K, in/out */, int idx_beg, int n_params, const double *drotv);
/* {Linear,Cubic}Trajectory::evaluate without the Jacobian (src/backend/trajectory.cpp:86-110 / :329-355) */
int cmx_traj_evaluate(int order, int K, const double *knots, int64_t start_ns, int64_t dt_ns, int64_t t_ns,
                      double quat_out[4]);
/* CMaxSLAM::precomputeBearingVectors (src/cmax_slam.cpp:106-120): lut[(y*W+x)*3..] = projectPixelTo3dRay(
 * rectifyPoint(x,y)) of image_geometry's pinhole model, plumb_bob D = k1 k2 p1 p2 k3.  K 3x3, R 3x3, P 3x4
 * row-major; D, R, P may be NULL (no distortion, identity, [K|0]).  image_geometry / cv::undistortPoints are not
 * vendored by the reference: restated from their documented behaviour, parity unpinned. */
int cmx_bearing_lut(int W, int H, const double K[9], const double D[5], const double R[9], const double P[12],
                    double *lut /* W*H*3 */);

/* ------------------------------------------------------------------ timing hooks ------------------------
 * HIP-event timing of the dominant kernels on the context's stream (bench.py's roofline leg).
 * cmx_timing_enable(ctx, mask) makes every evaluation record events around the kernel classes whose bit is set
 * (bit CMX_T_SPLAT, ...; 0xff = all, 0 = off); mask | (n << 8) samples every n-th evaluation only.  The per-event
 * kernels (splat, gather) carry their events on the kernel itself (hipExtLaunchKernelGGL start / stop: the dispatch's
 * own timestamps, the same rocprofv3 reports); the other classes are bracketed on the stream (CMX_T_COMM: the RCCL collectives of an attached communicator,
 * i.e. including the wait for the slowest rank);
 * cmx_timing_get returns accumulated milliseconds and launch counts per kernel class, then resets. */
enum { CMX_T_SPLAT = 0, CMX_T_IMAGE = 1, CMX_T_POSE = 2, CMX_T_GATHER = 3, CMX_T_ZERO = 4, CMX_T_COMM = 5, CMX_T_FINAL = 6, CMX_T_BATCH = 7, CMX_T_COUNT = 8 };
/* CMX_T_FINAL: the separate finalize launch (absent when CMX_OPT_TAIL_FINALIZE folds it into the last kernel);
 * CMX_T_BATCH: the back end's per-batch pass of the gradient gather.  Every class except CMX_T_ZERO / CMX_T_COMM is timed
 * through events carried by its (main) kernel: the dispatch's own begin / end timestamps, what rocprofv3 reports. */
/* cmx_get_stats: counters of a context, one double each, indexed by this enum (ABI 6: the indices have names; 0..16 keep the
 * values they had as bare numbers). */
enum {
  CMX_STAT_REBINS = 0,              /* destination-tile sorts so far */
  CMX_STAT_FALLBACK_FRAC = 1,       /* fraction of votes that left their LDS window in the last evaluation */
  CMX_STAT_CHUNKS = 2,              /* workgroup chunks of the current sort */
  CMX_STAT_EVENTS = 3,              /* packed (sub-sampled) events */
  CMX_STAT_REUSE_HITS = 4,          /* gradient evaluations that reused the resident image of the previous cost evaluation */
  CMX_STAT_SHARDED_HOST_SYNCS = 5,  /* host synchronisations between the splat and the last kernel of sharded evaluations (stays 0) */
  CMX_STAT_EXCHANGE_MISSES = 6,     /* sharded evaluations whose exchange set missed flagged tiles (completed by a second exchange) */
  CMX_STAT_EXCHANGE_TILES = 7,      /* tiles in the current exchange set (-1: none known, whole planes) */
  CMX_STAT_COMM_BYTES = 8,          /* bytes the last sharded evaluation exchanged (all collectives, this rank's buffers) */
  CMX_STAT_SPEC_IMAGES = 9,         /* cost-only evaluations that ran the adjoint image pass speculatively */
  CMX_STAT_SPEC_HITS = 10,          /* gradient evaluations that found it ready */
  CMX_STAT_GATED_LAUNCHES = 11,     /* gated gradient passes queued (cmx_hint_next_df) */
  CMX_STAT_GATED_HITS = 12,         /* gradient evaluations served by one */
  CMX_STAT_CHAIN_SOLVES = 13,       /* device-driven solves started */
  CMX_STAT_CHAIN_SLOTS = 14,        /* evaluation slots they queued */
  CMX_STAT_CHAIN_TAKEOVERS = 15,    /* solves the host took over (disagreement, or votes outside their windows in a fused slot) */
  CMX_STAT_CHAIN_WARM_STARTS = 16,  /* device-driven solves that started warm (nothing copied or cleared in front of them) */
  CMX_STAT_FUSED_EVALS = 17,        /* evaluations whose image pass ran inside the splat launch (two launches instead of three) */
  CMX_STAT_FUSED_REDOS = 18,        /* ... of which were repeated (votes beyond the reach of their tiles' arrival counts) */
  CMX_STAT_ONE_LAUNCH_EVALS = 19,   /* ... of which ran splat, image pass, gather and finalize as ONE launch */
  CMX_STAT_FUSED_TIMEOUTS = 20,     /* repeats caused by a tile workgroup that gave up waiting (stays 0: a wait is bounded at 2 ms) */
  CMX_STAT_SELF_SERVE_EVALS = 21,   /* ... of the one-launch evaluations, those of the self-service form (chunk workgroups alone) */
  CMX_STAT_HOST_FINALIZE_EVALS = 22, /* front-end gradient evaluations finalized on the host from per-shard records (CMX_OPT_TAIL_FINALIZE 4) */
  CMX_N_STATS = 23
};
int cmx_get_stats(cmx_ctx *ctx, double *stats, int n_stats); /* writes min(n_stats, CMX_N_STATS) entries (ABI 3: the length is explicit) */
/* ABI revision of this header: bumped whenever a signature or the layout of a caller-provided buffer changes
 * (3: cmx_get_stats takes the buffer length; cmx_frontend_prepare / cmx_backend_prepare added;
 *  4: groups, cmx_backend_get_pose_table, stream priority / CU mask;
 *  5: cmx_comm_info; the event store behind a group (cmx_events_create_group, cmx_backend_set_window_from on a group);
 *     CMX_OPT_SPIN_WAIT values >= 2 are a spin budget in microseconds for all three waiters (before: "spin"), negative values are
 *     rejected (before: accepted as non-zero);
 *  6: named cmx_get_stats indices, five more of them (the buffer length is the caller's: old callers keep reading what they asked for); cmx_group_transport_info; the *_aos entry points; cmx_set_stream_priority /
 *     cmx_set_cu_mask moved to cmax_hip_diag.h;
 *     added without a bump (no signature or buffer layout changed): the seven cmx_backend_recon_* entry points, then
 *     recon_restart / _contrast / _grad_add[_aos|_from] / _grad_get / _eval_from, then recon_bind_from / _unbind / _eval_bound /
 *     _bound_info, then recon_freeze_head / _frozen_info / _solve, then recon_extend / _bind_append_from / _advance_head /
 *     _release_head / _online_info and the value CMX_RECON_KEEP_HEAD of recon_solve's freeze_head; the entry points of the later features (recon_warp*, recon_pol_*,
 *     recon_view_*, recon_voxel_*, recon_surface_*, recon_score*) likewise; then cmx_events_select[_device] / _pixel_counts[_device] / _read with cmx_select) */
#define CMX_ABI_VERSION 6
int cmx_abi_version(void);
int cmx_timing_enable(cmx_ctx *ctx, int on);
int cmx_timing_get(cmx_ctx *ctx, double ms[CMX_T_COUNT], int64_t launches[CMX_T_COUNT]);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* CMAX_HIP_H */
