#!/usr/bin/env python
"""ROS-free end-to-end run: events in -> angular velocities -> trajectory + panoramic map out.

An EXAMPLE host around the drop-in evaluator, not part of the product: it replays, single-threaded and in the order
the reference's two threads would interleave on a recorded bag, the control logic the reference keeps in

    AngVelEstimator::pushEvent / slideWindow          src/frontend/ang_vel_estimator.cpp:68-183
    PoseGraphOptimizer::pushAngVel / Run / getEventSubset / getAngVelSubset / processTimeWindow / slideWindow
                                                      src/backend/pose_graph_optimizer.cpp:60-189, :244-376

and calls, for everything that is on the accelerated path or next to it,

    FrontendEvaluator.setupProblemAndOptimize   (cmx_frontend_solve)       one packet  -> omega
    trajectory.integrateAngVel / Trajectory.generateCtrlPoses              omegas      -> new control poses
    BackendEvaluator.setupProblemAndOptimize    (cmx_backend_solve)        one window  -> refined control poses
    BackendEvaluator.updateIG / setUpdateTimesIG                           map upkeep on the device
    EventStore                                                             events uploaded once, sliced on device

Usage:  python examples/rotation_pipeline.py [--seconds 1.2] [--rate 2e6] [--degree 1|3]
Prints the angular-velocity RMSE of the front end and the orientation error of dead reckoning vs the refined
trajectory against the synthetic ground truth.
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cmax_slam_amd import evaluator, synth, trajectory  # noqa: E402

NS = 1_000_000_000


def _dur_ns(sec):
    """ros::Duration(double): fromSec -> floor seconds + rounded nanoseconds."""
    s = int(np.floor(sec))
    return s * NS + int(round((sec - s) * 1e9))


class Params:
    """Defaults of launch/ecrot_synth.launch:12-41 (sensor-size dependent ones scaled by the caller)."""
    num_events_per_packet = 60000   # ~30 ms of the synthetic 2 Mev/s stream (ecrot_synth.launch:22 uses 70000)
    dt_ang_vel = 0.01
    event_batch_size = 100
    frontend_event_sample_rate = 1
    backend_event_sample_rate = 1
    frontend_blur_sigma = 1.0
    backend_blur_sigma = 1.0
    time_window_size = 0.2
    sliding_window_stride = 0.1
    spline_degree = 1
    dt_knots = 0.05
    pano_height = 512
    backend_min_ev_rate = 10000
    max_update_times = 200
    Y_angle = 0.0
    deterministic = False           # CMX_OPT_DETERMINISTIC on both contexts: the same bits on every run


def write_display_images(fe, be, ang_vel, pose, prefix, gamma=0.75):
    """The two images the reference publishes, tone-mapped on the device, as binary PGM / PPM files:
    <prefix>_local_iwe.pgm (raw | motion-compensated events of the packet `fe` holds) and <prefix>_pano.ppm (the resident
    map with the sensor outline at `pose`).  Returns the two paths."""
    pair = fe.publishEventImage(ang_vel)
    pano = be.publishEventImage(gamma, pose)
    paths = (prefix + "_local_iwe.pgm", prefix + "_pano.ppm")
    with open(paths[0], "wb") as f:
        f.write(b"P5\n%d %d\n255\n" % (pair.shape[1], pair.shape[0]) + pair.tobytes())
    with open(paths[1], "wb") as f:  # the image is BGR (cv::Mat order), a PPM is RGB
        f.write(b"P6\n%d %d\n255\n" % (pano.shape[1], pano.shape[0]) + np.ascontiguousarray(pano[..., ::-1]).tobytes())
    return paths


def _support_range(traj, t):
    """[first, last) of the events inside the knot support of the trajectory"""
    t_hi = traj.t_beg_ns + (traj.size() - traj.order + 1) * traj.dt_ns
    return int(np.searchsorted(t, traj.t_beg_ns, side="left")), int(np.searchsorted(t, t_hi, side="left"))


def refine_trajectory(be, traj, x, y, t, prm, store=None, bind=False, native=False, freeze_head=None):
    """One bundle adjustment over the WHOLE recording, the step a rotational event SLAM ends with once the sliding windows have
    passed: FR-CG over every control pose but the first order - 1 (a common rotation of all of them is a gauge freedom of the
    contrast), cost = -contrast of the panorama of all events along the trajectory: BackendEvaluator.reconstruct_refine
    (cmx_backend_recon_eval_from; bind=True: the events are bound once and every trial point is a cmx_backend_recon_eval_bound, votes
    through LDS over a tile sort kept between evaluations).  native=True: the same problem as ONE call, BackendEvaluator.reconstruct_solve
    (cmx_backend_recon_solve) over the bound events; freeze_head=N then fixes the first N control poses (N > order - 1: a settled head
    of the trajectory) and votes the event batches under them once.  Returns (refined knots, report); the report carries
    contrast_before / contrast_after."""
    i0, i1 = _support_range(traj, t)
    own = store is None
    if own:  # (the evaluation reads its events from a device-resident store)
        store = evaluator.EventStore(be.W, be.H, max(i1 - i0, 1))
        store.push(x[i0:i1], y[i0:i1], t[i0:i1])
        i0, i1 = 0, i1 - i0
    try:
        if native:
            be.reconstruct_begin(traj.order, traj.knots, traj.t_beg_ns, traj.dt_ns, prm.event_batch_size, prm.backend_event_sample_rate)
            try:
                be.reconstruct_bind(store, i0, i1 - i0)
                knots, rep = be.reconstruct_solve(traj.knots, traj.order - 1 if freeze_head is None else int(freeze_head),
                                                  sigma=prm.backend_blur_sigma, freeze_head=freeze_head is not None)
                if freeze_head is not None:
                    rep = dict(rep, **be.reconstruct_frozen_info())
            finally:
                be.reconstruct_end()
        else:
            knots, rep = be.reconstruct_refine(store, i0, i1 - i0, traj.order, traj.knots, traj.t_beg_ns, traj.dt_ns, traj.order - 1,
                                               sigma=prm.backend_blur_sigma, event_batch_size=prm.event_batch_size,
                                               event_sample_rate=prm.backend_event_sample_rate, bind=bind)
    finally:
        if own:
            store.close()
    rep = dict(rep, contrast_before=-rep["initial_cost"], contrast_after=-rep["final_cost"], events=i1 - i0)
    return knots, rep


def refine_trajectory_online(be, traj, x, y, t, prm, store, stride_s, free=8, log=None):
    """refine_trajectory(native=True) the way an online host runs it: the recording is replayed in strides of stride_s seconds, and
    per stride the spline grows (reconstruct_extend), the stride's events are appended to the binding (reconstruct_bind_append), the
    tail is solved under the frozen head as it stands (reconstruct_solve(freeze_head="keep")), the freeze line moves up to `free`
    knots behind the end (reconstruct_advance_head) and the settled events' memory is given back (reconstruct_release_head).  The cost
    of a stride follows its events, the memory the active tail.  Returns (refined knots, report); the report carries
    contrast_after, strides, iterations and resident_max, the largest number of sampled events resident after a release."""
    i0, i1 = _support_range(traj, t)
    K_all, order = traj.size(), traj.order
    stride = max(1, int(round(stride_s * 1e9 / traj.dt_ns)))
    knots = np.array(traj.knots, np.float64, copy=True)
    rep = dict(strides=0, iterations=0, resident_max=0, events=i1 - i0)
    K, done = min(K_all, order + free), i0
    try:
        while True:
            hi = int(np.searchsorted(t, traj.t_beg_ns + (K - order + 1) * traj.dt_ns, side="left")) if K < K_all else i1
            q = np.ascontiguousarray(knots[:K])
            if rep["strides"] == 0:
                be.reconstruct_begin(order, q, traj.t_beg_ns, traj.dt_ns, prm.event_batch_size, prm.backend_event_sample_rate)
                be.reconstruct_bind(store, done, hi - done)
                be.reconstruct_advance_head(order - 1)  # (the gauge: a head that freezes nothing yet)
            else:
                be.reconstruct_extend(q)
                be.reconstruct_bind_append(store, done, hi - done)
            nf = be.reconstruct_frozen_info()["num_fixed"]
            knots[:K], r = be.reconstruct_solve(q, nf, sigma=prm.backend_blur_sigma, freeze_head="keep")
            be.reconstruct_advance_head(max(nf, K - free))
            be.reconstruct_release_head()
            on = be.reconstruct_online_info()
            rep["strides"] += 1
            rep["iterations"] += r["iterations"]
            rep["resident_max"] = max(rep["resident_max"], on["resident_sampled"])
            if log:
                log("  stride %d: %d knots (%d fixed), %d new events, %d iterations, contrast %.6g; %d sampled events resident, %d released" %
                    (rep["strides"], K, nf, hi - done, r["iterations"], -r["final_cost"], on["resident_sampled"], on["released_sampled"]))
            done = hi
            if K == K_all:
                break
            K = min(K + stride, K_all)
        rep["contrast_after"] = be.reconstruct_eval_bound(None, prm.backend_blur_sigma, want_grad=False)[0]
    finally:
        be.reconstruct_end()
    return knots, rep


POLARITY_SEED = 2024  # --polarity-map: the synthetic stream's polarities are drawn, not modelled
HOT_FACTOR = 20.0  # --reject-outliers with --hot-pixels: a pixel with more than this many times the mean event count is masked
CROP_SIZE = (512, 384)  # --crop: the view's grid (a quarter of the sensor's field of view on about twice its pixels)


def reconstruct_panorama(be, traj, x, y, t, prm, store=None, knots=None):
    """All events inside the support of the refined trajectory, re-warped along the WHOLE of it (any number of control poses)
    into one panorama: BackendEvaluator.reconstruct_* (cmx_backend_recon_*).  Leaves the evaluator's window and map untouched.
    This function calls reconstruct_begin and adds the events, and returns with the reconstruction OPEN: the caller reads it with
    be.reconstruct_get() and / or be.reconstruct_render(), then closes it with be.reconstruct_end().
    knots: control poses to warp along instead of the trajectory's own (refine_trajectory's).
    Returns (first event, event count)."""
    i0, i1 = _support_range(traj, t)
    be.reconstruct_begin(traj.order, traj.knots if knots is None else knots, traj.t_beg_ns, traj.dt_ns, event_batch_size=prm.event_batch_size,
                         event_sample_rate=prm.backend_event_sample_rate)
    if store is not None:
        be.reconstruct_add_from(store, i0, i1 - i0)
    else:
        be.reconstruct_add(x[i0:i1], y[i0:i1], t[i0:i1])
    return i0, i1 - i0


def run_pipeline(stream, prm=None, use_event_store=True, log=None, display_prefix=None, reconstruct=False, refine_global=False,
                 refine_bound=False, refine_native=False, freeze_head=None, refine_online=None, online_free=8, export_warped=None,
                 polarity_map=None, frames=None, frame_ms=20.0, crop=None, voxels=None, voxel_ms=20.0, voxel_bins=5,
                 time_surfaces=None, surface_ms=20.0, surface_tau_ms=None, score_events=None, score_sigma=1.0, reject_outliers=None):
    """stream: synth.EventStream (or anything with x, y, t_ns, W, H, fx, fy, cx, cy, lut).  Returns a dict.
    display_prefix: write the final panorama with the last pose's FOV and the last packet's local-IWE pair there.
    reconstruct: after the last window, re-warp all events along the whole refined trajectory (res["recon"]; with
    display_prefix also <prefix>_recon.pgm).
    refine_global: after the last window, one bundle adjustment over the whole trajectory (res["refined_knots"],
    res["refine_report"]); the trajectory in res["traj"] stays the sliding windows' -- reconstruct then warps along the refined knots.
    refine_bound: that bundle adjustment binds the events once (reconstruct_refine(bind=True)).
    refine_native: it runs as one native call over the bound events (reconstruct_solve); freeze_head = N: with the first N control
    poses fixed and the batches under them voted once.
    refine_online = STRIDE_S: after that, the recording replayed in strides of STRIDE_S seconds through a binding that grows
    (refine_trajectory_online; res["online_knots"], res["online_report"]), with the last online_free control poses free.
    export_warped = PATH (implies reconstruct): where EVERY event of the reconstruction lands along the final trajectory, written to
    PATH.npz as xy (n x 2 panorama coordinates), flags (bit 0 sampled, bit 1 inside; 3 = the event voted) and index (the events'
    indices in the stream) -- what a host joins with whatever it kept per event; also res["warped"] = (index, xy, flags).
    polarity_map = PREFIX (implies reconstruct): the signed panorama ON - OFF of the same events along the final trajectory
    (BackendEvaluator.reconstruct_pol_*), written as PREFIX.pgm (OFF dark, ON bright) and PREFIX.ppm (ON red, OFF blue on white);
    also res["pol"] = (on, off).  The synthetic stream has no brightness model, so the polarities are DRAWN from a seeded generator
    (stream.polarity, when the stream has one, is used instead): the images show the arithmetic, not a scene's edges' signs.
    frames = PREFIX (implies reconstruct): the motion-compensated event frames of the final trajectory -- one pinhole view per
    frame_ms milliseconds with the sensor's size and intrinsics and the spline's pose at the slice centre
    (trajectory.frame_views, BackendEvaluator.reconstruct_view_*) -- written as PREFIX_0000.pgm ...; res["frames"] = (planes, counts).
    crop = PREFIX (implies reconstruct): one zoomed view of all events around the last pose, a quarter of the sensor's field of
    view on CROP_SIZE pixels (trajectory.crop_view), written as PREFIX.pgm; res["crop"] = (plane, count).
    voxels = PATH (implies reconstruct): the motion-compensated, polarity-signed voxel grids of the final trajectory -- one grid of
    voxel_bins time bins per voxel_ms milliseconds, with the sensor's size and intrinsics and the spline's pose at the slice centre
    (trajectory.voxel_grids, BackendEvaluator.reconstruct_voxel_*) -- written as one .npy of shape (G, B, H, W), the input format of
    event-based networks; res["voxels"] = (volumes, counts).  Polarities as for polarity_map.
    time_surfaces = PATH (implies reconstruct): the motion-compensated time surfaces of the final trajectory -- per surface_ms
    milliseconds one surface with the sensor's size and intrinsics and the spline's pose at the slice centre (trajectory.frame_views,
    BackendEvaluator.reconstruct_surface_*), ON and OFF channels, read through exp(-(t_hi - T) / tau) at its own t_hi with tau =
    surface_tau_ms (default: surface_ms) -- written as one .npy of shape (S, 2, H, W) fp32; res["time_surfaces"] = (decayed, counts).
    Polarities as for polarity_map.
    score_events = PATH (implies reconstruct): the support score of every event of the reconstruction against the final panorama,
    blurred with score_sigma (BackendEvaluator.reconstruct_score_*): the panorama read back where the event lands, an event that
    voted without its own vote -- many companions on a sharp edge, none for noise and hot pixels.  Written to PATH.npz as score
    (float32) and flags (as export_warped); res["scores"] = (score, flags).  The quartiles and the share of voting events with less
    than one vote of support are logged; nothing is asserted.
    reject_outliers = MIN_SCORE (implies reconstruct): after everything else, the voting events whose leave-one-out support (at
    score_sigma) is at least MIN_SCORE are selected ON THE DEVICE into a second store (EventStore.select on the scores' and flags'
    device tensors; host arrays without torch), the panorama is reconstructed again from the cleaned store and, with refine_native,
    the trajectory is solved again on it (reject_outliers_pass; res["reject"]).  A stream with hot pixels (stream.is_hot) also gets
    the share of their events removed and of the other events kept.  Logged; nothing is asserted."""
    reconstruct = (reconstruct or reject_outliers is not None or score_events is not None or export_warped is not None or polarity_map is not None or frames is not None or crop is not None
                   or voxels is not None or time_surfaces is not None)
    prm = prm or Params()
    x, y, t = stream.x, stream.y, stream.t_ns
    n_total = len(t)
    fe = evaluator.FrontendEvaluator(stream.W, stream.H, stream.lut)
    be = evaluator.BackendEvaluator(stream.W, stream.H, stream.lut, 2 * prm.pano_height, prm.pano_height)
    fe.set_fast_path()
    be.set_fast_path()
    if prm.deterministic:
        fe.set_deterministic(True)
        be.set_deterministic(True)
    pol = None
    if polarity_map is not None or voxels is not None or time_surfaces is not None:
        pol = getattr(stream, "polarity", None)
        pol = np.random.default_rng(POLARITY_SEED).integers(0, 2, n_total).astype(np.uint8) if pol is None else np.asarray(pol)
    store = None
    if use_event_store:
        store = evaluator.EventStore(stream.W, stream.H, n_total)
        store.push(x, y, t, polarity=pol)  # (with polarity: a byte array beside the events, which nothing but reconstruct_pol_add_from, reconstruct_voxel_add_from and
        # reconstruct_surface_add_from read)

    # ------------------------------------------------------------------ front end: packets (pushEvent)
    dt_av = _dur_ns(prm.dt_ang_vel)
    half = prm.num_events_per_packet // 2
    time_packet = int(t[0]) + _dur_ns(prm.dt_ang_vel * 0.5)
    time_get_subset = time_packet
    packets = []            # (idx_subset_beg, idx_subset_end, time_packet)
    subset_ts_map = []      # (event stamp, event index) -- ev_subset_ts_map_
    i = 0
    while True:
        # first event (not yet consumed) whose stamp exceeds the cursor
        i = max(i, int(np.searchsorted(t, time_get_subset, side="right")))
        if i >= n_total:
            break
        total = i + 1       # num_event_total_ after this event is appended
        packets.append((max(total - half, 0), total + half))
        subset_ts_map.append((int(t[i]), i))
        time_get_subset += dt_av
        i += 1
    ang_vel = np.zeros(3)
    ang_vels = []           # (time_packet, omega) pushed to the back end
    fe_ms = []
    for beg, end in packets:
        if n_total <= end:  # the reference waits for num_event_total_ > idx_subset_end: packet never completes
            break
        span = (int(t[end - 1]) - int(t[beg])) * 1e-9
        if span > 10 * prm.dt_ang_vel:
            ang_vel = np.zeros(3)
        else:
            t0 = time.perf_counter()
            args = (time_packet, stream.fx, stream.fy, stream.cx, stream.cy, prm.event_batch_size, prm.frontend_blur_sigma)
            if store is not None:
                fe.set_packet_from(store, beg, end - beg, *args)
            else:
                fe.set_packet(x[beg:end], y[beg:end], t[beg:end], *args)
            ang_vel, _rep = fe.setupProblemAndOptimize(ang_vel)
            fe_ms.append((time.perf_counter() - t0) * 1e3)
        ang_vels.append((time_packet, np.array(ang_vel, copy=True)))
        time_packet += dt_av
    if log:
        log("front end: %d packets, %.2f ms per packet (set + solve)" % (len(ang_vels), float(np.mean(fe_ms))))

    # ------------------------------------------------------------------ back end: sliding windows (Run)
    order = 2 if prm.spline_degree == 1 else 4
    win_size, win_stride = _dur_ns(prm.time_window_size), _dur_ns(prm.sliding_window_stride)
    cp_stride = int(round(prm.sliding_window_stride / prm.dt_knots))
    min_num_ev_per_win = (prm.time_window_size * prm.backend_min_ev_rate /
                          (prm.backend_event_sample_rate * prm.frontend_event_sample_rate))
    av_t = np.array([a[0] for a in ang_vels], np.int64)
    av_w = np.array([a[1] for a in ang_vels])
    map_t = np.array([m[0] for m in subset_ts_map], np.int64)
    map_i = np.array([m[1] for m in subset_ts_map], np.int64)
    # pushAngVel, first call
    t_win_beg = int(av_t[0]); t_win_end = t_win_beg + win_size
    t_av_beg, t_av_end = t_win_beg, t_win_end
    traj = trajectory.Trajectory(prm.spline_degree, t_win_beg, prm.dt_knots)
    ang_vel_prev = (int(av_t[0]), av_w[0].copy())
    th = prm.Y_angle * np.pi / 180
    pose_latest = (int(av_t[0]), _quat_from_matrix(np.array([[np.cos(th), 0, np.sin(th)], [0, 1, 0],
                                                             [-np.sin(th), 0, np.cos(th)]])))
    first_time_window, count_window, idx_cp_opt_beg = True, 0, 0
    av_used = 0             # frontend_ang_vel_.erase(begin, iter_end)
    dead_reckoning = [pose_latest]
    dr_pose = pose_latest
    dr_prev = ang_vel_prev
    reports, be_ms = [], []
    while av_t[-1] > t_win_end:  # isReadyFrontendPoses
        # getEventSubset(t_win_beg, t_win_end): packet-level search, then 100-event steps back from the end
        kb = int(np.searchsorted(map_t, t_win_beg, side="right"))
        ke = int(np.searchsorted(map_t, t_win_end, side="left"))
        if kb >= len(map_i) or ke >= len(map_i):
            break
        ev_beg, ev_end = int(map_i[kb]), int(map_i[ke])
        t_end_mod = t_win_end - _dur_ns(1e-6)
        while t[ev_end] > t_end_mod:
            ev_end -= 100
            if ev_end <= ev_beg:
                ev_end = ev_beg + 1
                break
        # getAngVelSubset(t_av_beg, t_av_end): stamps in (beg, end)
        a0 = max(int(np.searchsorted(av_t, t_av_beg, side="right")), av_used)
        a1 = int(np.searchsorted(av_t, t_av_end, side="left"))
        sub = (av_t[a0:a1], av_w[a0:a1])
        av_used = a1
        # processTimeWindow
        poses, ang_vel_prev = trajectory.integrateAngVel(pose_latest, sub, ang_vel_prev, first_time_window)
        dr_poses, dr_prev = trajectory.integrateAngVel(dr_pose, sub, dr_prev, first_time_window)
        if len(dr_poses[0]):
            dr_pose = (int(dr_poses[0][-1]), dr_poses[1][-1])
            dead_reckoning += list(zip(dr_poses[0].tolist(), dr_poses[1]))
        cps_new = traj.generateCtrlPoses(poses, t_av_beg, t_av_end)
        if first_time_window:
            idx_cp_opt_beg = 3 if prm.spline_degree == 3 else 1
            first_time_window = False
        else:
            cps_new = cps_new[(3 if prm.spline_degree == 3 else 1):]
        traj.pushbackCtrlPoses(cps_new)
        idx_cp_traj_beg = count_window * cp_stride
        idx_cp_opt_beg = max(idx_cp_traj_beg, idx_cp_opt_beg)
        num_cp_opt = traj.size() - idx_cp_opt_beg
        n_ev = ev_end - ev_beg
        if n_ev > min_num_ev_per_win:
            t0 = time.perf_counter()
            knots, start_ns, dt_ns = traj.temp_window(idx_cp_traj_beg)
            args = (order, knots, start_ns, dt_ns, idx_cp_opt_beg - idx_cp_traj_beg, t_win_beg + win_stride)
            kw = dict(event_batch_size=prm.event_batch_size, event_sample_rate=prm.backend_event_sample_rate,
                      blur_sigma=prm.backend_blur_sigma, IG="resident")  # the global map never leaves the device
            if store is not None:
                be.set_window_from(store, ev_beg, n_ev, *args, **kw)
            else:
                be.set_window(x[ev_beg:ev_end], y[ev_beg:ev_end], t[ev_beg:ev_end], *args, **kw)
            drotv, rep = be.setupProblemAndOptimize()
            traj.incrementalUpdate(drotv, idx_cp_opt_beg)
            be.updateIG(prm.max_update_times)
            # PoseGraphOptimizer::setUpdateTimesIG: FOV visit map every 0.05 s over the stride
            t_check = t_win_beg
            while t_check < t_win_beg + win_stride:
                be.setUpdateTimesIG(traj.evaluate(t_check), 3)
                t_check += _dur_ns(0.05)
            be_ms.append((time.perf_counter() - t0) * 1e3)
            reports.append(rep)
            assert num_cp_opt * 3 == len(drotv)
        t_latest = t_win_end - _dur_ns(1e-6)
        pose_latest = (t_latest, traj.evaluate(t_latest))
        # slideWindow
        t_win_beg += win_stride
        t_av_beg = t_win_end
        t_win_end += win_stride
        t_av_end = t_win_end
        count_window += 1
    if log:
        log("back end: %d windows, %.2f ms per window (set + solve + map upkeep)" % (len(reports), float(np.mean(be_ms))))
    if display_prefix and pose_latest is not None and len(av_w):
        paths = write_display_images(fe, be, av_w[-1], pose_latest[1], display_prefix)
        if log:
            log("display images: %s, %s" % paths)
    res = dict(ang_vel_t=av_t, ang_vel=av_w, traj=traj, dead_reckoning=dead_reckoning, IG=be.getIG(),
               reports=reports, fe_ms=fe_ms, be_ms=be_ms, windows=count_window)
    if refine_global and traj.size() >= traj.order:
        t0 = time.perf_counter()
        res["refined_knots"], res["refine_report"] = refine_trajectory(be, traj, x, y, t, prm, store, bind=refine_bound,
                                                                       native=refine_native, freeze_head=freeze_head)
        if log:
            r = res["refine_report"]
            log("global refinement: %d events, %d control poses, %d iterations (%d f, %d df) in %.2f ms; contrast %.6g -> %.6g" %
                (r["events"], traj.size(), r["iterations"], r["n_f"], r["n_df"], (time.perf_counter() - t0) * 1e3,
                 r["contrast_before"], r["contrast_after"]))
    if refine_online and traj.size() >= traj.order:
        t0 = time.perf_counter()
        own = store is None
        st = store
        if own:  # (the online path reads its events from a device-resident store; indices are the stream's)
            st = evaluator.EventStore(be.W, be.H, max(len(x), 1))
            st.push(x, y, t)
        try:
            res["online_knots"], res["online_report"] = refine_trajectory_online(be, traj, x, y, t, prm, st, refine_online, online_free, log)
        finally:
            if own:
                st.close()
        if log:
            r = res["online_report"]
            log("online refinement: %d events in %d strides of %.3g s, last %d control poses free: %d iterations in %.2f ms; contrast %.6g; "
                "at most %d sampled events resident" % (r["events"], r["strides"], refine_online, online_free, r["iterations"],
                                                         (time.perf_counter() - t0) * 1e3, r["contrast_after"], r["resident_max"]))
    if reconstruct and traj.size() >= traj.order:
        t0 = time.perf_counter()
        i_rec, n_rec = reconstruct_panorama(be, traj, x, y, t, prm, store, res.get("refined_knots"))
        res["recon"], n_sampled, n_inside = be.reconstruct_get(with_counts=True)
        if export_warped is not None:  # (the same range in one call: the batches are those of the vote loop above)
            if store is not None:
                xy, flags = be.reconstruct_warp_from(store, i_rec, n_rec)
            else:
                xy, flags = be.reconstruct_warp(x[i_rec:i_rec + n_rec], y[i_rec:i_rec + n_rec], t[i_rec:i_rec + n_rec])
            index = np.arange(i_rec, i_rec + n_rec, dtype=np.int64)
            res["warped"] = (index, xy, flags)
            np.savez(export_warped + ".npz", xy=xy, flags=flags, index=index)
            if log:
                log("export: %d events to %s.npz, %d of them voted" % (n_rec, export_warped, int(np.count_nonzero(flags == 3))))
        if score_events is not None:  # (the same range in one call, right after the votes: the own contribution is the event's)
            be.reconstruct_score_open(score_sigma)
            if store is not None:
                score, sflags = be.reconstruct_score_from(store, i_rec, n_rec, loo=True)
            else:
                score, sflags = be.reconstruct_score(x[i_rec:i_rec + n_rec], y[i_rec:i_rec + n_rec], t[i_rec:i_rec + n_rec], loo=True)
            res["scores"] = (score, sflags)
            np.savez(score_events + ".npz", score=score, flags=sflags)
            if log:
                voted = score[sflags == 3]
                q = np.percentile(voted, [25, 50, 75]) if len(voted) else np.zeros(3)
                log("scores: %d events to %s.npz at sigma %g; leave-one-out support of the %d voting events: quartiles %.2f / %.2f / %.2f, "
                    "%.1f %% below one vote" % (n_rec, score_events, score_sigma, len(voted), q[0], q[1], q[2],
                                                100.0 * float(np.mean(voted < 1.0)) if len(voted) else 0.0))
        if log:
            log("reconstruction: %d events along %d control poses in %.2f ms (%d sampled, %d voted)" %
                (n_rec, traj.size(), (time.perf_counter() - t0) * 1e3, n_sampled, n_inside))
        if display_prefix:
            img = be.reconstruct_render(0.75)
            with open(display_prefix + "_recon.pgm", "wb") as f:
                f.write(b"P5\n%d %d\n255\n" % (img.shape[1], img.shape[0]) + img.tobytes())
        if polarity_map is not None:  # (the same range in one call again, under the knots the count panorama was voted at)
            t0 = time.perf_counter()
            if store is not None:
                be.reconstruct_pol_add_from(store, i_rec, n_rec)
            else:
                be.reconstruct_pol_add(x[i_rec:i_rec + n_rec], y[i_rec:i_rec + n_rec], t[i_rec:i_rec + n_rec], pol[i_rec:i_rec + n_rec])
            on, off, n_on, n_off = be.reconstruct_pol_get(with_counts=True)
            res["pol"] = (on, off)
            mono, bgr = be.reconstruct_pol_render(0.75, 0), be.reconstruct_pol_render(0.75, 1)
            with open(polarity_map + ".pgm", "wb") as f:
                f.write(b"P5\n%d %d\n255\n" % (mono.shape[1], mono.shape[0]) + mono.tobytes())
            with open(polarity_map + ".ppm", "wb") as f:  # (PPM is RGB)
                f.write(b"P6\n%d %d\n255\n" % (bgr.shape[1], bgr.shape[0]) + np.ascontiguousarray(bgr[:, :, ::-1]).tobytes())
            if log:
                log("polarity map: %d ON and %d OFF events voted in %.2f ms -> %s.pgm, %s.ppm" %
                    (n_on, n_off, (time.perf_counter() - t0) * 1e3, polarity_map, polarity_map))
        knots_rec = traj.knots if res.get("refined_knots") is None else res["refined_knots"]

        def view_votes(views, Wv, Hv):  # (the same range in one call again, under the knots the count panorama was voted at)
            be.reconstruct_view_begin(views, Wv, Hv)
            if store is not None:
                be.reconstruct_view_add_from(store, i_rec, n_rec)
            else:
                be.reconstruct_view_add(x[i_rec:i_rec + n_rec], y[i_rec:i_rec + n_rec], t[i_rec:i_rec + n_rec])
            planes, counts = be.reconstruct_view_get(with_counts=True)
            images = [be.reconstruct_view_render(k, 0.75) for k in range(len(views))]
            be.reconstruct_view_end()
            return planes, counts, images

        def write_pgm(path, img):
            with open(path, "wb") as f:
                f.write(b"P5\n%d %d\n255\n" % (img.shape[1], img.shape[0]) + img.tobytes())

        if frames is not None:  # one de-rotated frame per frame_ms of the events the reconstruction holds, seen by the sensor itself
            t0 = time.perf_counter()
            views = trajectory.frame_views(traj.order, knots_rec, traj.t_beg_ns, traj.dt_ns, int(round(frame_ms * 1e6)),
                                           (stream.fx, stream.fy, stream.cx, stream.cy), t_beg_ns=int(t[i_rec]),
                                           t_end_ns=int(t[i_rec + n_rec - 1]) + 1)
            planes, counts, images = view_votes(views, stream.W, stream.H)
            res["frames"] = (planes, counts)
            for k, img in enumerate(images):
                write_pgm("%s_%04d.pgm" % (frames, k), img)
            if log:
                log("frames: %d motion-compensated frames of %.3g ms, %d to %d events each, in %.2f ms -> %s_0000.pgm ..." %
                    (len(views), frame_ms, int(counts.min()), int(counts.max()), (time.perf_counter() - t0) * 1e3, frames))
        if crop is not None:  # all events around the last pose, at a quarter of the sensor's field of view on a grid of its own
            t_last = traj.t_beg_ns + (traj.size() - traj.order + 1) * traj.dt_ns - 1
            final = trajectory.Trajectory(prm.spline_degree, traj.t_beg_ns, prm.dt_knots)
            final.pushbackCtrlPoses(knots_rec)
            q_last = final.evaluate(t_last)
            fov = np.degrees(2 * np.arctan(0.5 * stream.W / stream.fx)) / 4
            planes, counts, images = view_votes([trajectory.crop_view(q_last, fov, CROP_SIZE[0], CROP_SIZE[1])], *CROP_SIZE)
            res["crop"] = (planes[0], int(counts[0]))
            write_pgm(crop + ".pgm", images[0])
            if log:
                log("crop: %d events within %.1f degrees around the last pose on %d x %d -> %s.pgm" %
                    (int(counts[0]), fov, CROP_SIZE[0], CROP_SIZE[1], crop))
        if voxels is not None:  # the signed event volume a network reads: grids of voxel_ms x voxel_bins seen by the sensor itself
            t0 = time.perf_counter()
            grids = trajectory.voxel_grids(traj.order, knots_rec, traj.t_beg_ns, traj.dt_ns, int(round(voxel_ms * 1e6)),
                                           (stream.fx, stream.fy, stream.cx, stream.cy), t_beg_ns=int(t[i_rec]),
                                           t_end_ns=int(t[i_rec + n_rec - 1]) + 1)
            be.reconstruct_voxel_begin(grids, stream.W, stream.H, voxel_bins, signed=True)
            if store is not None:
                be.reconstruct_voxel_add_from(store, i_rec, n_rec)
            else:
                be.reconstruct_voxel_add(x[i_rec:i_rec + n_rec], y[i_rec:i_rec + n_rec], t[i_rec:i_rec + n_rec], pol[i_rec:i_rec + n_rec])
            volumes, counts = be.reconstruct_voxel_get(with_counts=True)
            be.reconstruct_voxel_end()
            res["voxels"] = (volumes, counts)
            path = voxels if voxels.endswith(".npy") else voxels + ".npy"
            np.save(path, volumes)
            if log:
                log("voxels: %d grids of %.3g ms x %d bins, %d to %d events each, in %.2f ms -> %s %s" %
                    (len(grids), voxel_ms, voxel_bins, int(counts.min()), int(counts.max()), (time.perf_counter() - t0) * 1e3, path,
                     volumes.shape))
        if time_surfaces is not None:  # when every scene point last fired, per polarity: one surface per surface_ms, decayed at its end
            t0 = time.perf_counter()
            views = trajectory.frame_views(traj.order, knots_rec, traj.t_beg_ns, traj.dt_ns, int(round(surface_ms * 1e6)),
                                           (stream.fx, stream.fy, stream.cx, stream.cy), t_beg_ns=int(t[i_rec]),
                                           t_end_ns=int(t[i_rec + n_rec - 1]) + 1)
            tau_ms = surface_ms if surface_tau_ms is None else surface_tau_ms
            be.reconstruct_surface_begin(views, stream.W, stream.H, by_polarity=True)
            if store is not None:
                be.reconstruct_surface_add_from(store, i_rec, n_rec)
            else:
                be.reconstruct_surface_add(x[i_rec:i_rec + n_rec], y[i_rec:i_rec + n_rec], t[i_rec:i_rec + n_rec], pol[i_rec:i_rec + n_rec])
            decayed = be.reconstruct_surface_decay(tau_ms * 1e6)
            counts = be.reconstruct_surface_get(0, len(views), with_counts=True)[1]
            be.reconstruct_surface_end()
            res["time_surfaces"] = (decayed, counts)
            path = time_surfaces if time_surfaces.endswith(".npy") else time_surfaces + ".npy"
            np.save(path, decayed)
            if log:
                log("time surfaces: %d of %.3g ms, tau %.3g ms, %d to %d events each, in %.2f ms -> %s %s" %
                    (len(views), surface_ms, tau_ms, int(counts.min()), int(counts.max()), (time.perf_counter() - t0) * 1e3, path,
                     decayed.shape))
        if reject_outliers is not None:
            be.reconstruct_restart(knots_rec)  # (whatever ran above, the count panorama of the whole range once more)
            st = store
            if st is None:  # (the selection reads its events from a device-resident store)
                st = evaluator.EventStore(be.W, be.H, max(n_rec, 1))
                st.push(x[i_rec:i_rec + n_rec], y[i_rec:i_rec + n_rec], t[i_rec:i_rec + n_rec])
            first = i_rec if store is not None else 0
            try:
                res["reject"] = reject_outliers_pass(be, traj, st, first, n_rec, prm, float(reject_outliers), score_sigma, knots_rec,
                                                     getattr(stream, "is_hot", None), i_rec, refine_native, log)
            finally:
                if store is None:
                    st.close()
        else:
            be.reconstruct_end()
    return res


def reject_outliers_pass(be, traj, store, first, count, prm, min_score, score_sigma, knots, is_hot, i_stream, refine, log):
    """--reject-outliers: with the reconstruction begun and empty, vote store[first, first+count), score every event against the
    panorama (leave-one-out, blurred with score_sigma), SELECT the voting events with score >= min_score into a second store on the
    device (EventStore.select: the events never leave it; device tensors when torch is importable, host arrays otherwise),
    reconstruct again from the cleaned store and, with refine, solve the trajectory again on it.  Closes the reconstruction.
    A stream that says it has hot pixels (is_hot) also gets a sensor mask from the per-pixel event counts of the range
    (EventStore.pixel_counts): a pixel with more than HOT_FACTOR times the mean count is dropped -- a hot pixel's events line up
    along the camera's own path and support each other, so the score alone keeps them.
    Returns a dict: kept, share, contrast_before / _after (variance contrast at sigma 1), recon (the cleaned panorama), and with hot
    pixels in the stream hot_removed / hot_removed_by_score / others_kept, with refine knots + report.  It reports; nothing is asserted."""
    try:
        import torch
    except ImportError:
        torch = None
    out = {}
    clean = evaluator.EventStore(be.W, be.H, max(count, 1))
    try:
        be.reconstruct_add_from(store, first, count)
        out["contrast_before"] = be.reconstruct_contrast(1.0)
        be.reconstruct_score_open(score_sigma)
        pixel_keep = None
        mask_hot = is_hot is not None and np.any(is_hot)
        if torch is not None:
            if mask_hot:
                d_c = torch.empty((be.H, be.W), dtype=torch.int32, device="cuda")
                torch.cuda.synchronize()
                store.pixel_counts(first, count, out=d_c)
                pixel_keep = (d_c.double() <= HOT_FACTOR * count / (be.W * be.H)).to(torch.uint8).contiguous()
                torch.cuda.synchronize()
            d_s = torch.empty(count, dtype=torch.float32, device="cuda")
            d_f = torch.empty(count, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            be.reconstruct_score_from(store, first, count, loo=True, out=(d_s, d_f))
            kept = clean.select(store, first, count, score=d_s, min_score=min_score, flags=d_f, pixel_keep=pixel_keep)
        else:
            if mask_hot:
                pixel_keep = (store.pixel_counts(first, count) <= HOT_FACTOR * count / (be.W * be.H)).astype(np.uint8)
            s, f = be.reconstruct_score_from(store, first, count, loo=True)
            kept = clean.select(store, first, count, score=s, min_score=min_score, flags=f, pixel_keep=pixel_keep)
        out["kept"], out["share"] = kept, kept / max(count, 1)
        be.reconstruct_restart(knots)
        be.reconstruct_add_from(clean, 0, kept)
        out["recon"] = be.reconstruct_get()
        out["contrast_after"] = be.reconstruct_contrast(1.0)
        be.reconstruct_end()
        if log:
            log("outlier rejection: %d of %d events kept (%.1f %%) at leave-one-out support >= %g (%s form); variance contrast at "
                "sigma 1: %.6g -> %.6g" % (kept, count, 100.0 * out["share"], min_score, "device" if torch is not None else "host",
                                          out["contrast_before"], out["contrast_after"]))
        if mask_hot:  # (which events went: the same predicate in numpy, on host copies of the criteria)
            hot = np.asarray(is_hot[i_stream:i_stream + count], bool)
            if torch is not None:
                s, f, pixel_keep = d_s.cpu().numpy(), d_f.cpu().numpy(), pixel_keep.cpu().numpy()
            ex, ey = store.read(first, count)[:2]
            keep = (s >= np.float32(min_score)) & ((f & 3) == 3) & (pixel_keep.reshape(-1)[ey.astype(np.int64) * be.W + ex] != 0)
            by_score = (s >= np.float32(min_score)) & ((f & 3) == 3)  # (what the score and the flags alone would have kept)
            out["hot_removed"] = float(np.mean(~keep[hot])) if hot.any() else 0.0
            out["hot_removed_by_score"] = float(np.mean(~by_score[hot])) if hot.any() else 0.0
            out["others_kept"] = float(np.mean(keep[~hot])) if (~hot).any() else 0.0
            if log:
                log("  hot pixels: %.1f %% of their %d events removed (%.1f %% by the score and flags alone, the rest by the pixel mask), "
                    "%.1f %% of the other events kept" %
                    (100.0 * out["hot_removed"], int(hot.sum()), 100.0 * out["hot_removed_by_score"], 100.0 * out["others_kept"]))
        if refine and kept > 0:
            t_clean = clean.read(0, kept)[2]
            out["knots"], out["report"] = refine_trajectory(be, traj, None, None, t_clean, prm, clean, native=True)
            if log:
                r = out["report"]
                log("  refinement on the cleaned store: %d events, %d iterations; contrast %.6g -> %.6g" %
                    (r["events"], r["iterations"], r["contrast_before"], r["contrast_after"]))
    finally:
        be.reconstruct_end()
        clean.close()
    return out


def _quat_from_matrix(R):
    """Eigen::Quaterniond(R) for a rotation about Y (enough for R0)."""
    th = np.arctan2(R[0, 2], R[0, 0])
    return np.array([0.0, np.sin(th / 2), 0.0, np.cos(th / 2)])


def _angle_between(qa, qb):
    d = np.abs(np.sum(np.asarray(qa) * np.asarray(qb), axis=-1))
    return 2 * np.arccos(np.clip(d, 0, 1))


def _rel(q0, q):
    """q0^-1 * q for (x,y,z,w) arrays."""
    from scipy.spatial.transform import Rotation as Rot
    return (Rot.from_quat(q0).inv() * Rot.from_quat(q)).as_quat()


def evaluate_against_truth(stream, res):
    """Angular-velocity RMSE and orientation errors (both trajectories aligned to the truth at their first stamp)."""
    w_true = stream.omega_at(res["ang_vel_t"])
    w_err2 = np.sum((res["ang_vel"] - w_true) ** 2, axis=1)
    w_rmse = float(np.sqrt(np.mean(w_err2)))
    # the first solves start from omega = 0 (ang_vel_estimator.cpp:26) and need a few packets to lock on
    steady = res["ang_vel_t"] > res["ang_vel_t"][0] + 150_000_000
    w_rmse_steady = float(np.sqrt(np.mean(w_err2[steady]))) if steady.any() else w_rmse
    traj = res["traj"]
    t_lo = traj.t_beg_ns
    t_hi = t_lo + (traj.size() - traj.order + 1) * traj.dt_ns - 1
    ts = np.arange(t_lo, t_hi, 10_000_000, dtype=np.int64)
    q_est = np.array([traj.evaluate(int(tt)) for tt in ts])
    q_gt = stream.quat_at(ts)
    err_ba = _angle_between(_rel(q_est[0], q_est), _rel(q_gt[0], q_gt))
    dr_t = np.array([p[0] for p in res["dead_reckoning"]], np.int64)
    dr_q = np.array([p[1] for p in res["dead_reckoning"]])
    keep = dr_t <= t_hi
    dr_gt = stream.quat_at(dr_t[keep])
    err_dr = _angle_between(_rel(dr_q[0], dr_q[keep]), _rel(dr_gt[0], dr_gt))
    return dict(omega_rmse=w_rmse, omega_rmse_steady=w_rmse_steady, ba_err_deg_rms=float(np.rad2deg(np.sqrt(np.mean(err_ba ** 2)))),
                ba_err_deg_max=float(np.rad2deg(err_ba.max())),
                dr_err_deg_rms=float(np.rad2deg(np.sqrt(np.mean(err_dr ** 2)))),
                dr_err_deg_max=float(np.rad2deg(err_dr.max())))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=1.2)
    ap.add_argument("--rate", type=float, default=2e6)
    ap.add_argument("--degree", type=int, default=1, choices=(1, 3))
    ap.add_argument("--host-events", action="store_true", help="re-upload events per packet/window (no EventStore)")
    ap.add_argument("--deterministic", action="store_true", help="bitwise reproducible evaluations (CMX_OPT_DETERMINISTIC)")
    ap.add_argument("--display", metavar="PREFIX", default=None,
                    help="write PREFIX_pano.ppm (final panorama, last pose's FOV) and PREFIX_local_iwe.pgm (one local-IWE pair)")
    ap.add_argument("--reconstruct", action="store_true",
                    help="after the last window, re-warp ALL events along the whole refined trajectory (with --display: PREFIX_recon.pgm)")
    ap.add_argument("--export-warped", metavar="PATH", default=None,
                    help="after the final refinement, write PATH.npz: the panorama coordinate (xy) and flags of every event warped along "
                         "the whole trajectory, and the events' indices (implies --reconstruct)")
    ap.add_argument("--score-events", metavar="PATH", default=None,
                    help="after the reconstruction (or any refine mode), write PATH.npz: the leave-one-out support score of every event "
                         "against the final panorama (score) and its flags; prints the quartiles and the share of voting events with "
                         "less than one vote of support (implies --reconstruct)")
    ap.add_argument("--reject-outliers", type=float, metavar="MIN_SCORE", default=None,
                    help="after the reconstruction (or any refine mode), select the voting events with leave-one-out support >= MIN_SCORE "
                         "into a second event store on the device, reconstruct again from it and print the kept share and the variance "
                         "contrast before and after; with --refine-native also solve again on the cleaned store (implies --reconstruct)")
    ap.add_argument("--hot-pixels", type=int, metavar="N", default=0,
                    help="N hot pixels fire 2 %% of the events each; --reject-outliers then prints how many of their events it removed")
    ap.add_argument("--score-sigma", type=float, default=1.0, help="blur of the panorama the scores are read from (0: none)")
    ap.add_argument("--polarity-map", metavar="PREFIX", default=None,
                    help="after the reconstruction, write the signed panorama ON - OFF as PREFIX.pgm and PREFIX.ppm (implies "
                         "--reconstruct).  The synthetic stream has no brightness model: the polarities are drawn from a seeded "
                         "random generator, so the images demonstrate the calls, not a scene")
    ap.add_argument("--frames", metavar="PREFIX", default=None,
                    help="after the reconstruction, write the motion-compensated event frames of the final trajectory as "
                         "PREFIX_0000.pgm ... (implies --reconstruct)")
    ap.add_argument("--frame-ms", type=float, metavar="MS", default=20.0, help="with --frames: the frame period in milliseconds")
    ap.add_argument("--crop", metavar="PREFIX", default=None,
                    help="after the reconstruction, write one zoomed view of all events around the last pose as PREFIX.pgm "
                         "(implies --reconstruct)")
    ap.add_argument("--voxels", metavar="PATH", default=None,
                    help="after the reconstruction, write the motion-compensated, polarity-signed voxel grids of the final trajectory "
                         "as ONE .npy of shape (G, B, H, W) (implies --reconstruct; polarities as for --polarity-map)")
    ap.add_argument("--voxel-ms", type=float, metavar="MS", default=20.0, help="with --voxels: the time range of a grid in milliseconds")
    ap.add_argument("--voxel-bins", type=int, metavar="B", default=5, help="with --voxels: time bins per grid, 1 to 64")
    ap.add_argument("--time-surfaces", metavar="PATH", default=None,
                    help="after the reconstruction, write the motion-compensated time surfaces of the final trajectory, decayed at "
                         "each surface's own end, as ONE .npy of shape (S, 2, H, W) fp32 (implies --reconstruct; polarities as for "
                         "--polarity-map)")
    ap.add_argument("--surface-ms", type=float, metavar="MS", default=20.0, help="with --time-surfaces: the time range of a surface in milliseconds")
    ap.add_argument("--surface-tau-ms", type=float, metavar="MS", default=None,
                    help="with --time-surfaces: the decay constant in milliseconds (default: --surface-ms)")
    ap.add_argument("--refine-global", action="store_true",
                    help="after the last window, one bundle adjustment over the whole trajectory (--reconstruct then uses its result)")
    ap.add_argument("--refine-bound", action="store_true",
                    help="with --refine-global: bind the events once and evaluate every trial point over the bound copy")
    ap.add_argument("--refine-native", action="store_true",
                    help="with --refine-global: the bundle adjustment as one native call over the bound events (cmx_backend_recon_solve)")
    ap.add_argument("--freeze-head", type=int, metavar="N", default=None,
                    help="with --refine-native: fix the first N control poses and vote the event batches under them once")
    ap.add_argument("--refine-online", type=float, metavar="STRIDE_S", default=None,
                    help="after the usual pipeline, replay the recording in strides of STRIDE_S seconds through a binding that grows: "
                         "extend, append, solve under the kept head, advance and release per stride")
    ap.add_argument("--online-free", type=int, metavar="N", default=8, help="with --refine-online: the last N control poses stay free")
    a = ap.parse_args()
    if a.freeze_head is not None and not a.refine_native:
        ap.error("--freeze-head needs --refine-native")
    if a.refine_online is not None and (a.refine_online <= 0 or a.online_free < 1):
        ap.error("--refine-online takes a stride > 0 and --online-free at least 1")
    if not a.frame_ms > 0:
        ap.error("--frame-ms must be > 0")
    if not a.voxel_ms > 0 or not 1 <= a.voxel_bins <= 64:
        ap.error("--voxel-ms must be > 0 and --voxel-bins in [1, 64]")
    if not a.surface_ms > 0 or (a.surface_tau_ms is not None and not a.surface_tau_ms > 0):
        ap.error("--surface-ms and --surface-tau-ms must be > 0")
    stream = synth.event_stream(a.rate, a.seconds, 240, 180, 200.0, 200.0, 119.5, 89.5, omega_mean=(0.2, 1.8, 0.3),
                                omega_amp=(1.0, 0.8, 1.0), hot_pixels=a.hot_pixels, hot_share=0.02 * a.hot_pixels)
    prm = Params()
    prm.spline_degree = a.degree
    prm.deterministic = a.deterministic
    t0 = time.perf_counter()
    res = run_pipeline(stream, prm, use_event_store=not a.host_events, log=print, display_prefix=a.display, reconstruct=a.reconstruct,
                       refine_global=a.refine_global or a.refine_native, refine_bound=a.refine_bound, refine_native=a.refine_native,
                       freeze_head=a.freeze_head, refine_online=a.refine_online, online_free=a.online_free, export_warped=a.export_warped,
                       polarity_map=a.polarity_map, frames=a.frames, frame_ms=a.frame_ms, crop=a.crop, voxels=a.voxels, voxel_ms=a.voxel_ms,
                       voxel_bins=a.voxel_bins, time_surfaces=a.time_surfaces, surface_ms=a.surface_ms, surface_tau_ms=a.surface_tau_ms,
                       score_events=a.score_events, score_sigma=a.score_sigma, reject_outliers=a.reject_outliers)
    wall = time.perf_counter() - t0
    m = evaluate_against_truth(stream, res)
    print("%.2f s of events (%d) processed in %.2f s wall" % (a.seconds, len(stream.x), wall))
    print("front end  |omega - truth| rmse      : %.4f rad/s (%.4f after the first 0.15 s)" % (m["omega_rmse"], m["omega_rmse_steady"]))
    print("dead reckoning orientation error    : rms %.3f deg, max %.3f deg" % (m["dr_err_deg_rms"], m["dr_err_deg_max"]))
    print("refined trajectory orientation error: rms %.3f deg, max %.3f deg" % (m["ba_err_deg_rms"], m["ba_err_deg_max"]))
    print("map: %d x %d, %.0f%% of pixels touched" % (res["IG"].shape[1], res["IG"].shape[0],
                                                       100.0 * float((res["IG"] > 0).mean())))
    if "refined_knots" in res:
        r = res["refine_report"]
        res["traj"].knots = res["refined_knots"]
        m2 = evaluate_against_truth(stream, res)
        print("global refinement: contrast %.6g -> %.6g; orientation error rms %.3f deg -> %.3f deg" %
              (r["contrast_before"], r["contrast_after"], m["ba_err_deg_rms"], m2["ba_err_deg_rms"]))
    if "online_knots" in res:
        r = res["online_report"]
        res["traj"].knots = res["online_knots"]
        m3 = evaluate_against_truth(stream, res)
        print("online refinement: contrast %.6g; orientation error rms %.3f deg -> %.3f deg; at most %d sampled events resident of %d" %
              (r["contrast_after"], m["ba_err_deg_rms"], m3["ba_err_deg_rms"], r["resident_max"], r["events"]))
    if "knots" in res.get("reject", {}):
        res["traj"].knots = res["reject"]["knots"]
        m4 = evaluate_against_truth(stream, res)
        print("refinement on the cleaned store: orientation error rms %.3f deg -> %.3f deg" % (m["ba_err_deg_rms"], m4["ba_err_deg_rms"]))
    if "recon" in res:
        print("reconstruction along the whole trajectory: %.0f votes, %.0f%% of pixels touched" %
              (float(res["recon"].sum(dtype=np.float64)), 100.0 * float((res["recon"] > 0).mean())))


if __name__ == "__main__":
    main()
