"""Schedules of the growing whole-trajectory binding's tests (tests/test_gpu_recon_online.py), shared and read-only;
tests/test_recon_online_cpu.py checks on the CPU that none of them is an empty comparison.

A schedule is a list of (K, num_fixed) per step over a configuration of recon_cases.py: at step i the spline has K_i knots, the
recording is cut at the end of their support, start + (K_i - order + 1) dt, and -- after the evaluations of the step -- the first
num_fixed_i knots are settled.  Knots: recon_grad_cases.point(name), the true spline perturbed by N(0, 0.01 rad) per knot; at
every step the knots that are not settled yet are moved again by N(0, 0.002 rad), seeded, so that every step evaluates at knots no
earlier step has seen while the settled ones keep their bytes."""
import functools

import numpy as np

import recon_cases as rc
import recon_grad_cases as rg

SCHEDULES = {
    "A": [(40, 20), (70, 50), (100, 80)],
    "B": [(30, 12), (50, 30), (70, 55)],
    "batch1": [(6, 4), (8, 5), (10, 7)],
    "batch3": [(6, 4), (8, 5), (10, 7)],
    "batch5000": [(6, 4), (8, 5), (10, 7)],
}
# (case, step) at which the advance freezes nothing new: batch5000's batches are longer than a knot interval's events
NOTHING_NEW = {("batch5000", 0), ("batch5000", 2)}
MOVE = 0.002


def cut(name, K):
    """events of the configuration's stream inside the support of its first K knots"""
    c, (w, x, y, t) = rc.CASES[name], rc.window(name)
    return int(np.searchsorted(t, w.start_ns + (K - c["order"] + 1) * w.dt_ns, side="left"))


@functools.lru_cache(maxsize=None)
def knots(name):
    """[the K_i knots of step i]: settled knots keep their bytes from step to step, the others move (read-only)"""
    out, prev, fixed = [], None, 0
    for i, (K, nf) in enumerate(SCHEDULES[name]):
        q = np.array(rg.point(name)[:K], copy=True)
        q[fixed:] = rg.perturb(q[fixed:], 7000 + 10 * rc.CASES[name]["seed"] + i, MOVE)
        if prev is not None:
            q[:fixed] = prev[:fixed]
        q = np.ascontiguousarray(q)
        q.setflags(write=False)
        out.append(q)
        prev, fixed = q, nf
    return out


def frozen_batches(name, n, K, nf):
    """(frozen batches, all batches) of the first n events under a spline of K knots with the first nf fixed: the prefix rule,
    restated -- batch pose times from the stream (midpoint of first and last event), segment s, s + order - 1 < nf"""
    c, (w, x, y, t) = rc.CASES[name], rc.window(name)
    if n < 2:
        return 0, 0
    B = c["batch"]
    nb = (n - 1 + B - 1) // B
    lo = np.arange(nb, dtype=np.int64) * B
    hi = np.where(n - lo > B, lo + B, n)
    tb = t[lo] + (t[hi - 1] - t[lo]) // 2  # (to a nanosecond of the library's rounding: no case sits on a boundary)
    s = np.minimum((tb - w.start_ns) // w.dt_ns, K - c["order"])
    active = np.nonzero(s + c["order"] - 1 >= nf)[0]
    return (int(active[0]) if len(active) else nb), nb


def sampled_in(name, n, batches):
    """sampled events in the first `batches` batches of the first n events"""
    c = rc.CASES[name]
    per_batch = (c["batch"] + c["rate"] - 1) // c["rate"]
    nb = (n - 1 + c["batch"] - 1) // c["batch"] if n > 1 else 0
    return batches * per_batch if batches < nb else rc.sampled(n, c["batch"], c["rate"])
