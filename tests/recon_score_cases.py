"""The references of the per-event support score tests (tests/test_gpu_recon_score.py; checked on the CPU by
tests/test_recon_score_cpu.py), in numpy:

  score32 / self0_32 / loo32   the fp32 EMULATION: float32 operations in the order include/cmax_hip.h states -- every product and every
                               sum rounded on its own -- from a support plane S and fp64 panorama coordinates (px, py).  What the
                               device's scores are compared with BIT FOR BIT, on the device's own S and its own exported coordinates.
  support_ref / self_ref       the fp64 REFERENCE: S = Gy plane Gx^T and self = w^T (Gy (x) Gx) w from the dense (or banded) REFLECT_101
                               operators of tests/dense_image_ops.py.
  self_closed                  the closed form of the own contribution, (wx^T Gx wx)(wy^T Gy wy) with Gx[a, b] = g(a - b) + the taps
                               that fold onto b, written out from the taps alone (no operator matrix): what the kernel evaluates.

and the two BORDER configurations.  A configuration of tests/recon_cases.py looks at the middle of the panorama; these take the same
kind of stream and pre-rotate knot i by a pitch of alpha_i about the camera's x axis, alpha running from 90 to 270 degrees over the
trajectory: the field of view starts on one pole, crosses the +-180 degree seam half way and ends on the other pole, so votes land
within the blur radius of all four borders of the plane (near a pole the field of view holds every azimuth, the seam's two sides
included).  events_with_fold counts, per border, the voting events whose own contribution contains a folded tap; the CPU test asserts
at least MIN_FOLDED for every border, for sigma 1 and 2.  Should a seed ever fail that, or put more than
recon_warp_cases.MAX_NEAR_INTEGER events within NEAR_INTEGER of a cell boundary, choose another seed: neither cap is to be changed."""
import functools
import math

import numpy as np

import dense_image_ops as dio
import recon_cases as rc
import recon_warp_cases as wc
from cmax_slam_amd import synth
from oracle import iwe_numpy
from oracle import pyoracle as po

F32 = np.float32
SIGMAS = (1.0, 2.0)
MIN_FOLDED = 20

# name -> as recon_cases.CASES
BORDER = {
    "sweep130x96": dict(N=30_000, Wp=130, Hp=96, order=4, K=40, batch=100, rate=1, seed=31),
    "sweep256x128": dict(N=40_000, Wp=256, Hp=128, order=4, K=40, batch=100, rate=1, seed=32),
}


def _qmul(a, b):
    """Hamilton product of (x, y, z, w) quaternions"""
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx,
                     aw * bz + ax * by - ay * bx + az * bw, aw * bw - ax * bx - ay * by - az * bz])


@functools.lru_cache(maxsize=None)
def case(name):
    """(cfg, window, x, y, t, knots) of a recon_cases configuration or of a border configuration; the arrays are read-only"""
    if name in rc.CASES:
        w, x, y, t = rc.window(name)
        return rc.CASES[name], w, x, y, t, w.knots_true
    c = BORDER[name]
    W, H, fx, fy, cx, cy = rc.SENSOR
    w = synth.backend_window(c["N"], W, H, fx, fy, cx, cy, c["Wp"], c["Hp"], c["order"], c["K"], 0, (c["K"] - c["order"] + 1) * rc.DT,
                             dt_knots=rc.DT, seed=c["seed"], knot_sigma=0.02)
    alpha = np.deg2rad(np.linspace(90.0, 270.0, c["K"]))
    knots = np.stack([_qmul(np.array([math.sin(a / 2), 0.0, 0.0, math.cos(a / 2)]), q) for a, q in zip(alpha, w.knots_true)])
    x, y, t = w.x.copy(), w.y.copy(), w.t_ns.copy()
    for a in (x, y, t, knots):
        a.setflags(write=False)
    return c, w, x, y, t, knots


def reference_of(name, x, y, t):
    """(px[n], py[n], flags[n]) of ONE call over (x, y, t): recon_warp_cases.reference_of for any configuration of case()"""
    c, w, _, _, _, knots = case(name)
    if name in rc.CASES:
        return wc.reference_of(po, name, x, y, t)
    W = rc.SENSOR[0]
    Wp, Hp, B, rate = c["Wp"], c["Hp"], c["batch"], c["rate"]
    x = np.asarray(x, np.int64); y = np.asarray(y, np.int64); t = np.asarray(t, np.int64)
    n = len(x)
    tp = wc.pose_times(t, B)
    times, inv = np.unique(tp, return_inverse=True)
    Rs = np.stack([iwe_numpy.q_to_R(po.spline_eval(c["order"], knots, w.start_ns, w.dt_ns, int(tb), jac=False)[0]) for tb in times])
    R = Rs[inv]
    bv = np.asarray(w.lut, np.float64).reshape(-1, 3)[y * W + x]
    ray = (R[:, :, 0] * bv[:, 0:1] + R[:, :, 1] * bv[:, 1:2]) + R[:, :, 2] * bv[:, 2:3]
    fx = (Wp / 360.0) * 180.0 / math.pi
    fy = (Hp / 180.0) * 180.0 / math.pi
    px, py, _ = iwe_numpy._project_equirect(ray, fx, fy, Wp / 2.0, Hp / 2.0)
    xx, yy = np.trunc(px).astype(np.int64), np.trunc(py).astype(np.int64)
    inside = (1 <= xx) & (xx < Wp - 2) & (1 <= yy) & (yy < Hp - 2)
    i = np.arange(n)
    _, lone = wc.batches(n, B)
    sampled = ((i - (i // B) * B) % rate == 0) & (i != lone)
    return px, py, (sampled * wc.SAMPLED + inside * wc.INSIDE).astype(np.uint8)


_refs = {}


def reference(name):
    """the reference coordinates and flags of the configuration's whole stream (computed once, read-only)"""
    if name not in _refs:
        _, _, x, y, t, _ = case(name)
        out = reference_of(name, x, y, t)
        for a in out:
            a.setflags(write=False)
        _refs[name] = out
    return _refs[name]


def cells(px, py):
    """(xx, yy int64, dx, dy float32) as the vote takes them from a coordinate: (int)p and (float)(p - (int)p)"""
    xx, yy = np.trunc(px).astype(np.int64), np.trunc(py).astype(np.int64)
    return xx, yy, (px - xx).astype(F32), (py - yy).astype(F32)


def plane64(px, py, flags, Hp, Wp):
    """the votes of the events with flags == 3 summed in fp64 (the fp32 weights, an exact sum up to fp64 rounding)"""
    m = flags == 3
    xx, yy, dx, dy = cells(px[m], py[m])
    w = iwe_numpy._weights(dx, dy).astype(np.float64)
    P = np.zeros((Hp, Wp))
    for k, (oy, ox) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
        np.add.at(P, (yy + oy, xx + ox), w[:, k])
    return P


# ---------------------------------------------------------------- fp32 emulation
def score32(S, px, py, flags):
    """score (no leave-one-out) of every event: fp32, ((w00 S00 + w01 S01) + w10 S10) + w11 S11 where INSIDE, else 0"""
    S = np.asarray(S)
    assert S.dtype == F32
    out = np.zeros(len(px), F32)
    m = (flags & wc.INSIDE) != 0
    xx, yy, dx, dy = cells(px[m], py[m])
    w = iwe_numpy._weights(dx, dy)
    assert w.dtype == F32
    s = ((w[:, 0] * S[yy, xx] + w[:, 1] * S[yy, xx + 1]) + w[:, 2] * S[yy + 1, xx]) + w[:, 3] * S[yy + 1, xx + 1]
    assert s.dtype == F32
    out[m] = s
    return out


def self0_32(px, py):
    """the own contribution at sigma 0 of every event (as if it voted): fp32, ((w00^2 + w01^2) + w10^2) + w11^2"""
    _, _, dx, dy = cells(px, py)
    w = iwe_numpy._weights(dx, dy)
    s = ((w[:, 0] * w[:, 0] + w[:, 1] * w[:, 1]) + w[:, 2] * w[:, 2]) + w[:, 3] * w[:, 3]
    assert s.dtype == F32
    return s


def loo32(score, self_term, flags):
    """leave-one-out: one fp32 subtraction for the events that voted (flags == 3), the score as it is for all others"""
    return np.where(flags == 3, (score - self_term).astype(F32), score).astype(F32)


# ---------------------------------------------------------------- fp64 reference
def taps_of(sigma):
    return np.asarray(po.gauss_kernel(sigma), F32).astype(np.float64)


def support_ref(plane, sigma):
    """S = Gy plane Gx^T in fp64 (sigma 0: the plane)"""
    return dio.blurred(plane, sigma) if sigma > 0 else np.asarray(plane, np.float64)


def support_bound(plane, sigma, ref):
    """(absolute per-pixel bound, e32): 8 max(e32, 2^-24) max |ref| with e32 the error of the SAME operators applied in fp32 relative
    to max |ref| -- dense_image_ops.bound's rule for the forward blur.  Nothing in it comes from a device's S."""
    A = np.asarray(plane, F32)
    o = dio._operators(A.shape[0], A.shape[1], sigma, F32)
    s32 = dio.apply2(o["Gy"], o["Gx"], A)
    assert s32.dtype == F32
    scale = float(np.abs(ref).max())
    e32 = float(np.abs(s32.astype(np.float64) - ref).max()) / scale if scale > 0 else 0.0
    return 8.0 * max(e32, dio.EPS32) * scale, e32


def _entry(M, a, b):
    """M[a, b] of a dense array or a Banded, element-wise over index arrays"""
    if isinstance(M, dio.Banded):
        d = b - a + M.b
        ok = (d >= 0) & (d <= 2 * M.b)
        return np.where(ok, M.band[a, np.clip(d, 0, 2 * M.b)], 0.0)
    return M[a, b]


def self_ref(px, py, Hp, Wp, sigma, exact_products=False):
    """w^T (Gy (x) Gx) w of every event over its four cells, from the operator matrices, in fp64.  w: the four fp32 vote weights --
    what the event added to the plane -- or, exact_products, the same products of the fp32 factors 1 - dx, dx, 1 - dy, dy formed in
    fp64 (the closed form's w, which factors exactly)"""
    xx, yy, dx, dy = cells(px, py)
    w = iwe_numpy._weights(dx, dy).astype(np.float64)
    if exact_products:
        ux, uy, vx, vy = ((F32(1) - dx).astype(np.float64), (F32(1) - dy).astype(np.float64), dx.astype(np.float64), dy.astype(np.float64))
        w = np.stack([ux * uy, vx * uy, ux * vy, vx * vy], axis=1)
    o = dio._operators(Hp, Wp, sigma, np.float64)
    off = ((0, 0), (0, 1), (1, 0), (1, 1))  # (oy, ox) of w00, w01, w10, w11
    out = np.zeros(len(px))
    for c, (cy, cx) in enumerate(off):
        for d, (ey, ex) in enumerate(off):
            out += w[:, c] * w[:, d] * _entry(o["Gx"], xx + cx, xx + ex) * _entry(o["Gy"], yy + cy, yy + ey)
    return out


def fold_entry(taps, L, a, b):
    """(Gx[a, b], folded) of the REFLECT_101 filter on a side of L > 2r + 1 cells: the tap g(a - b) plus every tap that folds onto b at
    the left border (position -b) or the right one (2 (L - 1) - b); folded: a tap was added"""
    r = (len(taps) - 1) // 2
    a, b = np.asarray(a), np.asarray(b)
    k0 = b - a + r
    g = np.where((k0 >= 0) & (k0 <= 2 * r), taps[np.clip(k0, 0, 2 * r)], 0.0)
    kl = r - a - b
    left = (kl >= 0) & (kl <= 2 * r) & (b > 0)
    kr = 2 * (L - 1) - a - b + r
    right = (kr >= 0) & (kr <= 2 * r) & (b < L - 1)
    g = g + np.where(left, taps[np.clip(kl, 0, 2 * r)], 0.0) + np.where(right, taps[np.clip(kr, 0, 2 * r)], 0.0)
    return g, left, right


def _axis_closed(taps, L, p, d):
    w = ((F32(1) - d).astype(np.float64), d.astype(np.float64))
    s = np.zeros(len(p))
    lo = np.zeros(len(p), bool)
    hi = np.zeros(len(p), bool)
    for i in (0, 1):
        for j in (0, 1):
            g, left, right = fold_entry(taps, L, p + i, p + j)
            s += w[i] * w[j] * g
            lo |= left
            hi |= right
    return s, lo, hi


def self_closed(px, py, Hp, Wp, sigma):
    """(self, fold) of every event: the closed form (wx^T Gx wx)(wy^T Gy wy) in fp64 with wx = (1 - dx, dx), wy = (1 - dy, dy) (fp32
    values), and fold = bool [n, 4]: a tap folded at the left, right, top, bottom border"""
    taps = taps_of(sigma)
    xx, yy, dx, dy = cells(px, py)
    sx, l, r_ = _axis_closed(taps, Wp, xx, dx)
    sy, t, b = _axis_closed(taps, Hp, yy, dy)
    return sx * sy, np.stack([l, r_, t, b], axis=1)


def events_with_fold(name, sigma):
    """voting events (flags == 3) per border -- left, right, top, bottom -- whose own contribution contains a folded tap"""
    c = case(name)[0]
    px, py, fl = reference(name)
    m = fl == 3
    _, fold = self_closed(px[m], py[m], c["Hp"], c["Wp"], sigma)
    return fold.sum(axis=0)


_planes = {}


def oracle_plane(name):
    """recon_cases.oracle_plane for any configuration of case(): ONE vote loop of the oracle over the whole stream (computed once)"""
    if name in rc.CASES:
        return rc.oracle_plane(po, name)
    if name not in _planes:
        c, w, x, y, t, knots = case(name)
        W, H = rc.SENSOR[:2]
        b = po.Backend(W, H, w.lut, c["Wp"], c["Hp"], c["order"], c["batch"], c["rate"], sigma=0.0)
        b.set_window(x, y, t, knots, w.start_ns, w.dt_ns, len(knots), 2 ** 62)
        p = b.accumulate_raw(np.zeros(0))[0].copy()
        p.setflags(write=False)
        _planes[name] = p
    return _planes[name]
