"""The reference of the pinhole-view tests (tests/test_gpu_recon_view.py): the planes and counters of a set of virtual pinhole
cameras over a recon_cases configuration, in numpy and fp64, built from pieces the suite already trusts --
recon_warp_cases.pose_times for batch membership and batch times, pyoracle.spline_eval + iwe_numpy.q_to_R for the batch rotation,
the bearing table, then the rules of include/cmax_hip.h:

  ray_w = R_batch bearing;  per view with t_lo <= batch time < t_hi:  v = R(quat)^T ray_w, iz = 1 / v.z, u = fx (v.x iz) + cx,
  w = fy (v.y iz) + cy;  the vote test v.z > 0 && 1 <= u < Wv-2 && 1 <= w < Hv-2;  cell (int)u, (int)w, fp32 weights

and iwe_numpy._weights / _add_votes for the votes, as recon_warp_cases.revote uses them.

tests/test_recon_view_cpu.py checks on the CPU that no view set is an empty comparison, that none puts more than
recon_warp_cases.MAX_NEAR_INTEGER voting events within NEAR_INTEGER of a cell boundary (should a set ever break that cap, replace
its seed here; the cap is not to be raised), and that the reference holds its own identities."""
import math

import numpy as np

import recon_cases as rc
import recon_warp_cases as wc
from oracle import iwe_numpy

W, H, FX, FY, CX, CY = rc.SENSOR
ALL_TIME = (-2 ** 62, 2 ** 62)

# name -> configuration, view size, kind of view set
SETS = {
    "frames8": dict(case="A", Wv=96, Hv=64, slices=8),
    "overlap40": dict(case="A", Wv=61, Hv=45, slices=40, widen=0.5),   # more views meet a run than one LDS chunk holds
    "full": dict(case="A", Wv=240, Hv=180, slices=0),                  # one view, all time, pose at mid-time
    "crop": dict(case="A", Wv=128, Hv=96, slices=3, zoom=2.5),       # the SENSOR's focal length x 2.5 on the smaller grid
    "linear": dict(case="B", Wv=96, Hv=64, slices=8),
    "batch1": dict(case="batch1", Wv=96, Hv=64, slices=5),
    "batch5000": dict(case="batch5000", Wv=96, Hv=64, slices=2),
    "n65": dict(case="n65", Wv=96, Hv=64, slices=1),
    "poles": dict(case="poles", Wv=96, Hv=64, slices=8),
    "shortest2": dict(case="shortest2", Wv=61, Hv=45, slices=4),
    # the full view turned about y.  180 degrees: every ray has v.z < 0.  90 degrees: the field of view (31 degrees to either side)
    # ends 59 degrees from the scene's centre, the scene 31 degrees plus a camera motion of ~0.2 rad from it: rays with v.z > 0
    # that all leave the plane.  45 degrees: a view that does receive votes past such rays.
    "behind": dict(case="A", Wv=240, Hv=180, slices=0, turned=(180.0, 90.0, 45.0)),
    # ten all-time views a few degrees apart: every run meets all of them, four LDS chunks with a partial last one
    "stack10": dict(case="A", Wv=61, Hv=45, slices=0, turned=tuple(3.0 * k for k in range(-5, 5))),
}
EDGE = ("n0", "n1", "n2")
EMPTY_VIEWS = {("behind", 0), ("behind", 1)}  # (set, view) expected to receive no vote


def scaled_intrinsics(Wv, Hv, zoom=None):
    """the sensor's intrinsics scaled to the view size, cx and cy offset by +0.25: no coordinate sits on a cell boundary;
    zoom: the focal length is the sensor's own times zoom instead"""
    sx, sy = Wv / W, Hv / H
    fx, fy = (FX * sx, FY * sy) if zoom is None else (zoom * FX, zoom * FY)
    return fx, fy, (CX + 0.5) * sx - 0.5 + 0.25, (CY + 0.5) * sy - 0.5 + 0.25


def q_mul(a, b):
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx,
                     aw * bz + ax * by - ay * bx + az * bw, aw * bw - ax * bx - ay * by - az * bz])


def spline_pose(po, case, t_ns, knots=None):
    c, w = rc.CASES[case], rc.window(case)[0]
    return po.spline_eval(c["order"], w.knots_true if knots is None else knots, w.start_ns, w.dt_ns, int(t_ns), jac=False)[0]


_sets = {}


def view_set(po, name):
    """(configuration, Wv, Hv, [(quat_xyzw, fx, fy, cx, cy, t_lo_ns, t_hi_ns), ...]) of a set: built once"""
    if name in _sets:
        return _sets[name]
    s = SETS[name]
    case, Wv, Hv = s["case"], s["Wv"], s["Hv"]
    _, x, y, t = rc.window(case)
    intr = scaled_intrinsics(Wv, Hv, s.get("zoom"))
    t0, t1 = int(t[0]), int(t[-1]) + 1
    views = []
    if s["slices"] == 0:
        q = spline_pose(po, case, t0 + (t1 - t0) // 2)
        turns = s.get("turned", (0.0,))
        for deg in turns:
            h = math.radians(deg) / 2
            views.append((q_mul(q, np.array([0.0, math.sin(h), 0.0, math.cos(h)])),) + intr + ALL_TIME)
    else:
        edges = [t0 + (t1 - t0) * i // s["slices"] for i in range(s["slices"] + 1)]
        for lo, hi in zip(edges[:-1], edges[1:]):
            q = spline_pose(po, case, lo + (hi - lo) // 2)
            pad = int(s.get("widen", 0.0) * (hi - lo))
            views.append((q,) + intr + (lo - pad, hi + pad))
    _sets[name] = (case, Wv, Hv, views)
    return _sets[name]


def edge_views(po, case):
    """one all-time view for the configurations with an edge count"""
    w = rc.window(case)[0]
    return [(np.array(w.knots_true[0]),) + scaled_intrinsics(96, 64) + ALL_TIME]


def world_rays(po, case, x, y, t, knots=None):
    """(ray_w[n, 3], pose time[n], sampled[n]) of ONE vote loop over (x, y, t): recon_warp_cases.reference_of up to the ray"""
    c, w = rc.CASES[case], rc.window(case)[0]
    B, rate = c["batch"], c["rate"]
    knots = w.knots_true if knots is None else knots
    x = np.asarray(x, np.int64); y = np.asarray(y, np.int64); t = np.asarray(t, np.int64)
    n = len(x)
    if n == 0:
        return np.zeros((0, 3)), np.zeros(0, np.int64), np.zeros(0, bool)
    tp = wc.pose_times(t, B)
    times, inv = np.unique(tp, return_inverse=True)
    Rs = np.stack([iwe_numpy.q_to_R(po.spline_eval(c["order"], knots, w.start_ns, w.dt_ns, int(tb), jac=False)[0]) for tb in times])
    R = Rs[inv]
    bv = np.asarray(w.lut, np.float64).reshape(-1, 3)[y * W + x]
    ray = (R[:, :, 0] * bv[:, 0:1] + R[:, :, 1] * bv[:, 1:2]) + R[:, :, 2] * bv[:, 2:3]
    i = np.arange(n)
    _, lone = wc.batches(n, B)
    sampled = ((i - (i // B) * B) % rate == 0) & (i != lone)
    return ray, tp, sampled


def project(view, ray, Wv, Hv):
    """(u, w, ok) of world rays in one view: the header's arithmetic, the test made in floating point"""
    q, fx, fy, cx, cy = np.asarray(view[0], np.float64), view[1], view[2], view[3], view[4]
    Rt = iwe_numpy.q_to_R(q / math.sqrt(float(np.sum(q * q)))).T
    v = (Rt[None, :, 0] * ray[:, 0:1] + Rt[None, :, 1] * ray[:, 1:2]) + Rt[None, :, 2] * ray[:, 2:3]
    with np.errstate(divide="ignore", invalid="ignore"):
        iz = 1.0 / v[:, 2]
        u = fx * (v[:, 0] * iz) + cx
        ww = fy * (v[:, 1] * iz) + cy
        ok = (v[:, 2] > 0) & (u >= 1) & (u < Wv - 2) & (ww >= 1) & (ww < Hv - 2)
    return u, ww, ok


def reference_of(po, case, views, Wv, Hv, x, y, t, knots=None):
    """(planes[M, Hv, Wv] fp32, counts[M] int64, members[M], near-integer voting events) of ONE view_add over (x, y, t)"""
    ray, tp, sampled = world_rays(po, case, x, y, t, knots)
    planes = np.zeros((len(views), Hv, Wv), np.float32)
    counts = np.zeros(len(views), np.int64)
    members = np.zeros(len(views), np.int64)
    near = 0
    for k, view in enumerate(views):
        m = sampled & (tp >= view[5]) & (tp < view[6])
        members[k] = int(np.count_nonzero(m))
        u, ww, ok = project(view, ray[m], Wv, Hv)
        u, ww = u[ok], ww[ok]
        counts[k] = len(u)
        near += int(np.count_nonzero(wc.near_integer(u, ww)))
        xx, yy = np.trunc(u).astype(np.int64), np.trunc(ww).astype(np.int64)
        dx, dy = (u - xx).astype(np.float32), (ww - yy).astype(np.float32)
        iwe_numpy._add_votes(planes[k], yy, xx, iwe_numpy._weights(dx, dy))
    return planes, counts, members, near


_refs = {}


def reference(po, name):
    """the reference of a set over its configuration's whole stream (computed once, read-only)"""
    if name not in _refs:
        case, Wv, Hv, views = view_set(po, name)
        _, x, y, t = rc.window(case)
        out = reference_of(po, case, views, Wv, Hv, x, y, t)
        for a in out[:3]:
            a.setflags(write=False)
        _refs[name] = out
    return _refs[name]


def still_camera(po, case):
    """(knots, view, expected plane, expected count): all knots equal, the view looks along them with the sensor's size and
    intrinsics (cx, cy + 0.25): every sampled event lands on its own pixel + 0.25, weights 0.75 / 0.25 per axis"""
    c, (w, x, y, t) = rc.CASES[case], rc.window(case)
    q = np.asarray(w.knots_true[len(w.knots_true) // 3], np.float64)
    knots = np.tile(q, (c["K"], 1))
    view = (q, FX, FY, CX + 0.25, CY + 0.25) + ALL_TIME
    n, B = c["N"], c["batch"]
    i = np.arange(n)
    sampled = ((i - (i // B) * B) % c["rate"] == 0) & (i != wc.batches(n, B)[1])
    xs, ys = np.asarray(x, np.int64)[sampled], np.asarray(y, np.int64)[sampled]
    m = (xs >= 1) & (xs < W - 2) & (ys >= 1) & (ys < H - 2)
    xs, ys = xs[m], ys[m]
    plane = np.zeros((H, W), np.float64)
    for oy, ox, wgt in ((0, 0, 0.75 * 0.75), (0, 1, 0.25 * 0.75), (1, 0, 0.75 * 0.25), (1, 1, 0.25 * 0.25)):
        np.add.at(plane, (ys + oy, xs + ox), wgt)
    return knots, view, plane, int(len(xs))


def views_meeting_a_run(po, name):
    """the largest number of views of a set whose range meets the batch times of one vote workgroup's run of packed events
    (cmx_recon.hip: recon_run(per_batch) = min(256 per_batch, 2048) packed events, starting at a multiple of itself)"""
    case, _, _, views = view_set(po, name)
    c = rc.CASES[case]
    t = rc.window(case)[3]
    B, rate = c["batch"], c["rate"]
    per_batch = (B + rate - 1) // rate
    run = min(256 * per_batch, 2048)
    tp = wc.pose_times(np.asarray(t, np.int64), B)
    nb = wc.batches(len(t), B)[0]
    bt = np.array([tp[b * B] for b in range(nb)], np.int64)
    n_packed = rc.sampled(len(t), B, rate)
    most = 0
    for e0 in range(0, n_packed, run):
        e1 = min(e0 + run, n_packed)
        span = bt[e0 // per_batch:(e1 - 1) // per_batch + 1]
        lo, hi = span.min(), span.max()
        most = max(most, sum(1 for v in views if v[5] <= hi and v[6] > lo))
    return most
