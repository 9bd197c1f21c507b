"""Evaluation points and CPU-oracle numbers of the whole-trajectory contrast / gradient tests (tests/test_gpu_recon_grad.py), built
once per process and shared; tests/test_recon_grad_inputs_cpu.py checks on the CPU that none of them is an empty comparison.

Evaluation point of a configuration (recon_cases.py): knots_true left-multiplied by exp(N(0, 0.01 rad)) per knot, seeded -- far from
a stationary point of the contrast.  Oracle numbers: pyoracle.Backend.eval at zero increments with num_fixed = 0, no map (alpha = 0)
and t_next_win_beg_ns = 2**62 (every event "old"): contrast of GaussianBlur(plane, sigma) and global_contrast_fdf's gradient with
respect to a left increment of every knot."""
import functools

import numpy as np

import recon_cases as rc

W, H = rc.SENSOR[:2]
PERTURB = 0.01

# the (case, sigma) pairs at which the fp32 oracle stays within 2.5e-6 of its all-fp64 build: RTOL is a fair bar there
SIGMA1 = ["A", "B", "batch1", "batch3", "batch5000", "n2", "n65", "pano130x96", "pano1000x300", "poles", "shortest4", "shortest2",
          "window"]
SIGMA02 = ["A", "B", "poles", "pano1000x300"]


# Seed of a configuration's evaluation point: 1000 + the configuration's own, except where the fp32 oracle at that point is itself
# further than 3e-6 from its all-fp64 build.  shortest4 (K = order: every event moves all four knots) is such a case at most seeds
# -- 1.1e-5 at 1011, 1.9e-5 at 2011, 5.9e-6 at 4011 -- and 2.3e-6 at 3011, measured on the oracle alone
# (tests/test_recon_grad_inputs_cpu.py holds every pair used to 3e-6).
POINT_SEED = {"shortest4": 3011}


def _quat_mul(a, b):
    ax, ay, az, aw = a.T
    bx, by, bz, bw = b.T
    return np.stack([aw * bx + ax * bw + ay * bz - az * by, aw * by + ay * bw + az * bx - ax * bz,
                     aw * bz + az * bw + ax * by - ay * bx, aw * bw - ax * bx - ay * by - az * bz], axis=1)


def perturb(knots, seed, sigma=PERTURB):
    """exp(d_k) * q_k with d_k ~ N(0, sigma) per component"""
    d = np.random.default_rng(seed).normal(0.0, sigma, (len(knots), 3))
    th = np.linalg.norm(d, axis=1, keepdims=True)
    e = np.concatenate([np.sin(th / 2) / th * d, np.cos(th / 2)], axis=1)
    q = _quat_mul(e, np.asarray(knots, np.float64))
    return np.ascontiguousarray(q / np.linalg.norm(q, axis=1, keepdims=True))


@functools.lru_cache(maxsize=None)
def point(name):
    """the evaluation point of a configuration (read-only)"""
    q = perturb(rc.window(name)[0].knots_true, POINT_SEED.get(name, 1000 + rc.CASES[name]["seed"]))
    q.setflags(write=False)
    return q


def oracle_eval(po, name, x, y, t, knots, sigma=1.0, measure=0, want_grad=True, exact=False, num_fixed=0, start_ns=None,
                side=2 ** 62):
    """(contrast, gradient over the knots from num_fixed on) of ONE vote loop over (x, y, t) along `knots`"""
    c, w = rc.CASES[name], rc.window(name)[0]
    cls = po.BackendExact if exact else po.Backend
    b = cls(W, H, w.lut, c["Wp"], c["Hp"], c["order"], c["batch"], c["rate"], sigma=float(sigma), measure=measure)
    b.set_window(x, y, t, knots, w.start_ns if start_ns is None else start_ns, w.dt_ns, num_fixed, side)
    return b.eval(np.zeros(3 * (len(knots) - num_fixed)), want_grad)


_refs = {}


def oracle_ref(po, name, sigma=1.0, measure=0):
    """(contrast, 3K gradient) of the oracle at the configuration's evaluation point over its whole stream (computed once)"""
    key = (name, float(sigma), int(measure))
    if key not in _refs:
        _, x, y, t = rc.window(name)
        c, g = oracle_eval(po, name, x, y, t, point(name), sigma, measure)
        g = np.array(g, copy=True)
        g.setflags(write=False)
        _refs[key] = (c, g)
    return _refs[key]


def rms_angle_deg(qa, qb):
    """rms over the knots of the angle of qa_k^-1 qb_k, degrees"""
    d = np.abs(np.sum(np.asarray(qa) * np.asarray(qb), axis=1)).clip(0, 1)
    return float(np.degrees(np.sqrt(np.mean((2 * np.arccos(d)) ** 2))))
