"""The configurations of the whole-trajectory reconstruction tests (tests/test_gpu_recon.py) and their CPU-oracle planes, built once
per process and shared; tests/test_recon_inputs_cpu.py checks on the CPU that none of them is an empty comparison.

Oracle plane of a configuration: pyoracle.Backend(..., sigma=0) with num_fixed = K and t_next_win_beg_ns = 2**62 (every event is
"old"), accumulate_raw at zero increments: IL_old is the vote loop of event_pano_warper.cpp:188-196 / :233-311 over the events,
for any K."""
import functools

import numpy as np

from cmax_slam_amd import synth

SENSOR = (240, 180, 200.0, 200.0, 119.5, 89.5)
DT = 0.05

# name -> N, pano, order, K, batch, rate, seed, knot_sigma.  T = the whole knot support (K - order + 1) * DT.
CASES = {
    "A": dict(N=60_007, Wp=512, Hp=256, order=4, K=100, batch=100, rate=1, seed=5),            # long cubic spline
    "B": dict(N=30_001, Wp=512, Hp=256, order=2, K=70, batch=64, rate=3, seed=6),              # linear, sub-sampled
    "batch1": dict(N=12_345, Wp=256, Hp=128, order=4, K=10, batch=1, rate=1, seed=7),          # batches far below a wave
    "batch3": dict(N=12_345, Wp=256, Hp=128, order=4, K=10, batch=3, rate=2, seed=7),
    "batch5000": dict(N=12_345, Wp=256, Hp=128, order=4, K=10, batch=5000, rate=1, seed=7),    # batches above a workgroup's run
    "n0": dict(N=0, Wp=256, Hp=128, order=4, K=10, batch=64, rate=1, seed=7),
    "n1": dict(N=1, Wp=256, Hp=128, order=4, K=10, batch=64, rate=1, seed=7),
    "n2": dict(N=2, Wp=256, Hp=128, order=4, K=10, batch=64, rate=1, seed=7),
    "n65": dict(N=65, Wp=256, Hp=128, order=4, K=10, batch=64, rate=1, seed=7),                # one batch + a skipped single event
    "pano130x96": dict(N=12_345, Wp=130, Hp=96, order=2, K=6, batch=100, rate=1, seed=8),
    "pano1000x300": dict(N=12_345, Wp=1000, Hp=300, order=4, K=10, batch=100, rate=1, seed=9),
    "poles": dict(N=12_345, Wp=256, Hp=128, order=4, K=40, batch=100, rate=1, seed=10, knot_sigma=0.15),  # votes dropped at the border
    "shortest4": dict(N=12_345, Wp=256, Hp=128, order=4, K=4, batch=100, rate=1, seed=11),     # K = order
    "shortest2": dict(N=12_345, Wp=256, Hp=128, order=2, K=2, batch=100, rate=1, seed=12),
    "window": dict(N=20_000, Wp=256, Hp=128, order=4, K=10, batch=100, rate=1, seed=13),       # also fits the window path (K <= 64)
}


def sampled(n, batch, rate):
    """events the sampling selects in ONE vote loop over n events: every batch restarts the stride; a trailing batch holding a
    single event is skipped (event_pano_warper.cpp:188-196, :262)"""
    if n < 2:
        return 0
    nb = (n - 1 + batch - 1) // batch
    last = min(batch, n - (nb - 1) * batch)
    return (nb - 1) * ((batch + rate - 1) // rate) + (last + rate - 1) // rate


@functools.lru_cache(maxsize=None)
def window(name):
    """the synthetic stream + true spline of a configuration; the event arrays are read-only"""
    c = CASES[name]
    W, H, fx, fy, cx, cy = SENSOR
    n_gen = max(c["N"], 200)  # (the generator wants a few events; the tiny cases take a prefix)
    w = synth.backend_window(n_gen, W, H, fx, fy, cx, cy, c["Wp"], c["Hp"], c["order"], c["K"], 0, (c["K"] - c["order"] + 1) * DT,
                             dt_knots=DT, seed=c["seed"], knot_sigma=c.get("knot_sigma", 0.02))
    x, y, t = w.x[:c["N"]].copy(), w.y[:c["N"]].copy(), w.t_ns[:c["N"]].copy()
    for a in (x, y, t, w.knots_true):
        a.setflags(write=False)
    return w, x, y, t


def oracle_loop(po, name, x, y, t, knots=None):
    """ONE vote loop of the oracle over (x, y, t) with the configuration's spline and sampling: a fresh (Hp, Wp) fp32 plane"""
    c = CASES[name]
    w = window(name)[0]
    W, H = SENSOR[:2]
    knots = w.knots_true if knots is None else knots
    b = po.Backend(W, H, w.lut, c["Wp"], c["Hp"], c["order"], c["batch"], c["rate"], sigma=0.0)
    b.set_window(x, y, t, knots, w.start_ns, w.dt_ns, len(knots), 2 ** 62)
    return b.accumulate_raw(np.zeros(0))[0].copy()


_planes = {}


def oracle_plane(po, name):
    """the oracle on the configuration's whole stream (computed once, read-only)"""
    if name not in _planes:
        _, x, y, t = window(name)
        p = oracle_loop(po, name, x, y, t)
        p.setflags(write=False)
        _planes[name] = p
    return _planes[name]


def cuts(name, *at):
    """[(lo, hi), ...] of the configuration's stream cut at the given event indices"""
    n = CASES[name]["N"]
    edges = [0] + list(at) + [n]
    return list(zip(edges[:-1], edges[1:]))
