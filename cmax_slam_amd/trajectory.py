"""Host-side mirror of the reference's trajectory bookkeeping around a back-end window.

Thin ctypes layer over the host C++ entry points of libcmaxhip.so (csrc/cmx_trajinit.cpp); names follow the
reference:

  integrateAngVel        PoseGraphOptimizer::integrateAngVel       src/backend/pose_graph_optimizer.cpp:191-222
  Trajectory             Linear/CubicTrajectory                    src/backend/trajectory.cpp, include/backend/trajectory.h
    .generateCtrlPoses   :205-214 / :480-489      .pushbackCtrlPoses   :81-84 / :324-327
    .incrementalUpdate   :221-238 / :491-499      .evaluate            :86-110 / :329-355
    .temp_window         what CopyAndIncrementalUpdate (:240-263 / :501-522) hands the event warper
  bearing_lut            CMaxSLAM::precomputeBearingVectors        src/cmax_slam.cpp:106-120

Nothing here touches the GPU; quaternions are (x, y, z, w) float64, stamps int64 ns.
"""
import ctypes as C

import numpy as np

from . import _lib
from .evaluator import CmaxHipError


def _chk(rc, what):
    if rc != _lib.OK:
        raise CmaxHipError(rc, "%s: %s" % (what, _lib.lib().cmx_status_string(rc).decode()))


def _d(a):
    return a.ctypes.data_as(_lib.c_dp)


def _i64(a):
    return a.ctypes.data_as(_lib.c_i64p)


def integrateAngVel(pose_latest, ang_vel_subset, ang_vel_prev, first_time_window):
    """pose_latest = (t_ns, quat); ang_vel_subset = (t_ns[n], omega[n,3]); ang_vel_prev = (t_ns, omega).
    Returns ((pose_t_ns[m], pose_quat[m,4]), ang_vel_prev')."""
    t = np.ascontiguousarray(ang_vel_subset[0], np.int64)
    w = np.ascontiguousarray(ang_vel_subset[1], np.float64).reshape(-1, 3)
    if len(t) != len(w):
        raise ValueError("ang_vel_subset: stamps and vectors differ in length")
    q0 = np.ascontiguousarray(pose_latest[1], np.float64)
    prev_t = np.array([int(ang_vel_prev[0])], np.int64)
    prev_w = np.array(ang_vel_prev[1], np.float64, copy=True)
    out_t = np.zeros(max(len(t), 1), np.int64)
    out_q = np.zeros((max(len(t), 1), 4))
    m = C.c_int(0)
    _chk(_lib.lib().cmx_integrate_ang_vel(len(t), _i64(t), _d(w), int(pose_latest[0]), _d(q0), _i64(prev_t), _d(prev_w),
                                          int(bool(first_time_window)), _i64(out_t), _d(out_q), C.byref(m)),
         "cmx_integrate_ang_vel")
    return (out_t[:m.value].copy(), out_q[:m.value].copy()), (int(prev_t[0]), prev_w)


def bearing_lut(W, H, K, D=None, R=None, P=None):
    K = np.ascontiguousarray(K, np.float64).reshape(9)
    opt = [None if a is None else np.ascontiguousarray(a, np.float64).reshape(n) for a, n in ((D, 5), (R, 9), (P, 12))]
    lut = np.zeros((H, W, 3))
    _chk(_lib.lib().cmx_bearing_lut(int(W), int(H), _d(K), *[None if a is None else _d(a) for a in opt], _d(lut)),
         "cmx_bearing_lut")
    return lut


class Trajectory:
    """Uniform cumulative B-spline on SO(3): spline_degree 1 -> order 2 (linear), 3 -> order 4 (cubic)."""

    def __init__(self, spline_degree, t_beg_ns, dt_knots):
        if spline_degree not in (1, 3):
            raise ValueError("spline_degree must be 1 or 3")
        self.order = 2 if spline_degree == 1 else 4
        self.t_beg_ns = int(t_beg_ns)                       # config.t_beg.toNSec()
        self.t_beg = _sec(self.t_beg_ns)                    # t_beg_ = config.t_beg.toSec()
        self.dt_knots = float(dt_knots)
        self.dt_ns = int(1e9 * self.dt_knots)               # int64_t(1e9 * config.dt_knots)
        self.knots = np.zeros((0, 4))

    def size(self):
        return len(self.knots)

    def generateCtrlPoses(self, poses, t_beg_ns, t_end_ns):
        """poses = (t_ns[m], quat[m,4]) -> new control poses fitted over [t_beg, t_end]."""
        n = _lib.lib().cmx_num_ctrl_poses(self.order, int(t_beg_ns), int(t_end_ns), self.dt_knots)
        t = np.ascontiguousarray(poses[0], np.int64)
        q = np.ascontiguousarray(poses[1], np.float64).reshape(-1, 4)
        out = np.zeros((max(n, 0), 4))
        _chk(_lib.lib().cmx_fit_ctrl_poses(self.order, len(t), _i64(t), _d(q), _sec(int(t_beg_ns)), self.dt_knots, n,
                                           _d(out)), "cmx_fit_ctrl_poses")
        return out

    def pushbackCtrlPoses(self, cps):
        self.knots = np.ascontiguousarray(np.vstack([self.knots, np.asarray(cps, np.float64).reshape(-1, 4)]))

    def incrementalUpdate(self, drotv, idx_beg):
        d = np.ascontiguousarray(drotv, np.float64).reshape(-1)
        _chk(_lib.lib().cmx_traj_incremental_update(self.size(), _d(self.knots), int(idx_beg), len(d), _d(d)),
             "cmx_traj_incremental_update")

    def evaluate(self, t_ns):
        q = np.zeros(4)
        _chk(_lib.lib().cmx_traj_evaluate(self.order, self.size(), _d(self.knots), self.t_beg_ns, self.dt_ns, int(t_ns),
                                          _d(q)), "cmx_traj_evaluate")
        return q

    def temp_window(self, idx_traj_beg):
        """(knots[idx_traj_beg:], start_ns, dt_ns) of the temporary trajectory the cost functor warps with; start_ns
        keeps the reference's double -> ns truncation (trajectory.cpp:255-256)."""
        start_ns = _lib.lib().cmx_traj_temp_start_ns(self.t_beg, int(idx_traj_beg), self.dt_knots)
        return np.ascontiguousarray(self.knots[idx_traj_beg:]), int(start_ns), self.dt_ns


def frame_views(order, knots, start_ns, dt_ns, period_ns, intrinsics, exposure_ns=None, t_beg_ns=None, t_end_ns=None):
    """The view list of a motion-compensated video (BackendEvaluator.reconstruct_view_begin): one _lib.ReconView per frame of
    period_ns over [t_beg_ns, t_end_ns) -- by default the whole knot support of the spline -- the last one cut at t_end_ns.
    A view's orientation is the spline's pose at the centre of its slice (cmx_traj_evaluate), its intrinsics are
    (fx, fy, cx, cy), and its time range is the slice, or exposure_ns around the slice centre (longer than the period: neighbouring
    frames share events; shorter: gaps)."""
    k = np.ascontiguousarray(knots, np.float64).reshape(-1, 4)
    start_ns, dt_ns, period_ns = int(start_ns), int(dt_ns), int(period_ns)
    if period_ns <= 0 or (exposure_ns is not None and int(exposure_ns) <= 0):
        raise ValueError("frame period and exposure must be > 0")
    t_beg = start_ns if t_beg_ns is None else int(t_beg_ns)
    t_end = start_ns + (len(k) - int(order) + 1) * dt_ns if t_end_ns is None else int(t_end_ns)
    fx, fy, cx, cy = intrinsics
    views = []
    q = np.zeros(4)
    for lo in range(t_beg, t_end, period_ns):
        hi = min(lo + period_ns, t_end)
        mid = lo + (hi - lo) // 2
        _chk(_lib.lib().cmx_traj_evaluate(int(order), len(k), _d(k), start_ns, dt_ns, mid, _d(q)), "cmx_traj_evaluate")
        if exposure_ns is not None:
            lo, hi = mid - int(exposure_ns) // 2, mid - int(exposure_ns) // 2 + int(exposure_ns)
        views.append(_lib.recon_view(q, fx, fy, cx, cy, lo, hi))
    return views


ALL_TIME_NS = (-2 ** 62, 2 ** 62)
# what a cell of a time surface holds when no event has reached it (BackendEvaluator.reconstruct_surface_get): INT64_MIN
SURFACE_EMPTY = -2 ** 63


def crop_view(quat_xyzw, fov_deg, Wv, Hv, t_range_ns=ALL_TIME_NS):
    """One view over all time (or t_range_ns) looking along quat_xyzw: a pinhole camera of Wv x Hv pixels whose horizontal field of
    view is fov_deg, principal point at the centre.  A field of view below the sensor's is a zoom: a crop of the scene on a finer
    grid than the sensor's or the panorama's."""
    if not 0.0 < float(fov_deg) < 180.0:
        raise ValueError("field of view must lie in (0, 180) degrees")
    f = 0.5 * Wv / np.tan(np.radians(float(fov_deg)) / 2)
    return _lib.recon_view(quat_xyzw, f, f, 0.5 * (Wv - 1), 0.5 * (Hv - 1), t_range_ns[0], t_range_ns[1])


def voxel_grids(order, knots, start_ns, dt_ns, period_ns, intrinsics, exposure_ns=None, t_beg_ns=None, t_end_ns=None):
    """The grid list of BackendEvaluator.reconstruct_voxel_begin: frame_views' list, one grid per slice of period_ns, oriented by the
    spline's pose at the slice centre.  A grid's bins divide its time range, so the range must be finite: one longer than 2^53 ns
    (ALL_TIME_NS, say, passed as t_beg_ns / t_end_ns or as the exposure) is refused here as the library refuses it."""
    n_knots = len(np.asarray(knots, np.float64).reshape(-1, 4))
    t_beg = int(start_ns) if t_beg_ns is None else int(t_beg_ns)
    t_end = int(start_ns) + (n_knots - int(order) + 1) * int(dt_ns) if t_end_ns is None else int(t_end_ns)
    for span in (t_end - t_beg, int(period_ns) if exposure_ns is None else int(exposure_ns)):
        if span > 2 ** 53:
            raise ValueError("a voxel grid needs a finite time range: at most 2^53 ns")
    return frame_views(order, knots, start_ns, dt_ns, period_ns, intrinsics, exposure_ns, t_beg_ns, t_end_ns)


def _sec(t_ns):
    """ros::Time::toSec()"""
    return float(t_ns // 1000000000) + 1e-9 * float(t_ns % 1000000000)
