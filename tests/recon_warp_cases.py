"""The per-event reference of the export tests (tests/test_gpu_recon_warp.py): where every event of a recon_cases configuration
lands, and its flags, in numpy -- built from pieces the oracle already has (iwe_numpy.batch_time_ns, pyoracle.spline_eval,
iwe_numpy.q_to_R and _project_equirect) with the batch, sampling and lone-event rules of include/cmax_hip.h:

  event i belongs to batch b = i // B and takes that batch's pose at the batch time; a trailing batch of exactly one event is no
  batch: that event takes the pose at its OWN time and is never SAMPLED; SAMPLED = (i - b B) % rate == 0; INSIDE = the vote test.

tests/test_recon_warp_cpu.py checks the reference against the oracle's vote loop before anything is compared with it.

A seed of recon_cases can be replaced here (SEEDS) should a configuration ever put more than MAX_NEAR_INTEGER events within
NEAR_INTEGER of a cell boundary; the cap is not to be raised."""
import math

import numpy as np

import recon_cases as rc
from oracle import iwe_numpy

SAMPLED, INSIDE = 1, 2
NEAR_INTEGER = 1e-9     # px: an event this close to an integer coordinate may fall into either cell
MAX_NEAR_INTEGER = 2    # ... and a configuration holds at most this many (expected: 4e-9 N, none)

# the configurations the export is compared on, and the ones with an edge count
CLOSURE = ("A", "B", "batch1", "batch3", "batch5000", "n65", "poles", "pano130x96", "shortest2", "shortest4")
EDGE = ("n0", "n1", "n2")
ALL = CLOSURE + EDGE
SEEDS = {}  # name -> seed replacing recon_cases' (none needed)


def window(name):
    assert name not in SEEDS  # (a replacement would build its own synth.backend_window here)
    return rc.window(name)


def batches(n, B):
    """(number of batches, index of the lone trailing event or -1) of ONE call over n events"""
    nb = (n - 1 + B - 1) // B if n > 1 else 0
    return nb, (n - 1 if n >= 1 and nb * B < n else -1)


def pose_times(t, B):
    """the time each event's pose is taken at"""
    n = len(t)
    nb, lone = batches(n, B)
    out = np.empty(n, np.int64)
    for b in range(nb):
        b0 = b * B
        b1 = b0 + B if n - b0 > B else n
        out[b0:b1] = iwe_numpy.batch_time_ns(t[b0], t[b1 - 1])
    if lone >= 0:
        out[lone] = t[lone]
    return out


def reference_of(po, name, x, y, t, knots=None):
    """(px[n], py[n], flags[n]) of ONE export call over (x, y, t) with the configuration's spline (or `knots`) and sampling"""
    c, w = rc.CASES[name], window(name)[0]
    W = rc.SENSOR[0]
    Wp, Hp, B, rate = c["Wp"], c["Hp"], c["batch"], c["rate"]
    knots = w.knots_true if knots is None else knots
    x = np.asarray(x, np.int64); y = np.asarray(y, np.int64); t = np.asarray(t, np.int64)
    n = len(x)
    if n == 0:
        return np.zeros(0), np.zeros(0), np.zeros(0, np.uint8)
    tp = pose_times(t, B)
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
    _, lone = batches(n, B)
    sampled = ((i - (i // B) * B) % rate == 0) & (i != lone)
    flags = (sampled * SAMPLED + inside * INSIDE).astype(np.uint8)
    return px, py, flags


_refs = {}


def reference(po, name):
    """the reference on the configuration's whole stream (computed once, read-only)"""
    if name not in _refs:
        _, x, y, t = window(name)
        out = reference_of(po, name, x, y, t)
        for a in out:
            a.setflags(write=False)
        _refs[name] = out
    return _refs[name]


def near_integer(px, py):
    """events the cell and flag comparisons may leave out: a coordinate within NEAR_INTEGER of an integer"""
    return (np.abs(px - np.rint(px)) < NEAR_INTEGER) | (np.abs(py - np.rint(py)) < NEAR_INTEGER)


def revote(px, py, flags, Hp, Wp):
    """the plane the events with flags == 3 vote, in event order, with the oracle's own vote functions"""
    m = flags == (SAMPLED | INSIDE)
    xx, yy = np.trunc(px[m]).astype(np.int64), np.trunc(py[m]).astype(np.int64)
    dx, dy = (px[m] - xx).astype(np.float32), (py[m] - yy).astype(np.float32)
    img = np.zeros((Hp, Wp), np.float32)
    iwe_numpy._add_votes(img, yy, xx, iwe_numpy._weights(dx, dy))
    return img
