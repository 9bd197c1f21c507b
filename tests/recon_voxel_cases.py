"""The reference of the voxel-grid tests (tests/test_gpu_recon_voxel.py): the polarity-signed, time-binned volumes of a set of grids
over a recon_cases configuration, in numpy, built from pieces the suite already trusts -- recon_view_cases.world_rays for batch
membership, batch pose and world ray, recon_view_cases.project for the view's projection and vote test, recon_pol_cases.polarity
for the events' polarity, iwe_numpy._weights / _add_votes for the fp32 bilinear products and the adds -- with the per-event rules
of include/cmax_hip.h:

  an event belongs to every grid with t_lo <= t_i < t_hi, t_i its OWN timestamp;  n_bins >= 2: scale = (n_bins - 1) / (t_hi - t_lo),
  tau = (double)(t_i - t_lo) * scale, b0 = min((int)tau, n_bins - 2), f = (float)(tau - b0), bin b0 gets wt = 1 - f and bin b0 + 1
  gets wt = f;  n_bins == 1: wt = 1;  every cell receives s * (wt * wb) in fp32, s = -1 for an OFF event of a signed set.

tests/test_recon_voxel_cpu.py checks on the CPU that no set is an empty comparison, that none puts more than
recon_warp_cases.MAX_NEAR_INTEGER voting events within NEAR_INTEGER of a cell boundary (should a set ever break that cap, replace
its seed or orientation here; the cap is not to be raised), and that the reference holds its own identities."""
import math

import numpy as np

import recon_cases as rc
import recon_pol_cases as pc
import recon_view_cases as vc
import recon_warp_cases as wc
from oracle import iwe_numpy

F32 = np.float32

# name -> configuration, grid size (96 x 64 unless given), bins, signedness and the kind of grid set
SETS = {
    "A5": dict(case="A", slices=3, bins=5),                       # the ordinary shape
    "B2": dict(case="B", slices=4, bins=2),                       # linear spline, sample rate 3, the smallest n_bins with weights
    "one_bin": dict(case="A", slices=8, bins=1, signed=False),    # no temporal weight at all
    "batch5000": dict(case="batch5000", slices=2, bins=4),        # a batch spans many bins and both grids
    "batch1": dict(case="batch1", slices=5, bins=3),
    # ten grids over the whole stream a few degrees apart: every run meets all of them, four LDS chunks with a partial last one
    "overlap10": dict(case="A", Wv=61, Hv=45, bins=2, turned=tuple(3.0 * k for k in range(-5, 5))),
    # one grid from exactly the timestamp of an event in mid-stream to exactly that of a later one
    "edges_in_time": dict(case="A", bins=3, between=(1 / 3, 2 / 3)),
    "n65": dict(case="n65", bins=2, support=True),                # the lone trailing event ...
    "n0": dict(case="n0", bins=2, support=True),                  # ... and the empty inputs
    "n1": dict(case="n1", bins=2, support=True),
    "n2": dict(case="n2", bins=2, support=True),
    "poles": dict(case="poles", slices=2, bins=2),                # rays behind the camera and off the plane
}
EDGE = ("n0", "n1", "n2")  # sets whose grid may stay empty

_sets = {}


def _voting_event_at(po, case, view, Wv, Hv, start):
    """the first event at or behind `start` that is sampled, later than its predecessor, and inside the view's plane"""
    _, x, y, t = rc.window(case)
    ray, _, sampled = vc.world_rays(po, case, x, y, t)
    _, _, ok = vc.project(view, ray, Wv, Hv)
    t = np.asarray(t, np.int64)
    for i in range(start, len(t)):
        if sampled[i] and ok[i] and t[i] > t[i - 1]:
            return i
    raise AssertionError("no voting event behind %d" % start)


def voxel_set(po, name):
    """(configuration, Wv, Hv, n_bins, signed, [(quat_xyzw, fx, fy, cx, cy, t_lo_ns, t_hi_ns), ...]) of a set: built once"""
    if name in _sets:
        return _sets[name]
    s = SETS[name]
    case, Wv, Hv = s["case"], s.get("Wv", 96), s.get("Hv", 64)
    w, x, y, t = rc.window(case)
    c = rc.CASES[case]
    intr = vc.scaled_intrinsics(Wv, Hv)
    grids = []
    if s.get("support"):  # the whole knot support, looking along the first knot (recon_view_cases.edge_views)
        grids.append((np.array(w.knots_true[0]),) + intr + (int(w.start_ns), int(w.start_ns + (c["K"] - c["order"] + 1) * w.dt_ns)))
    elif "between" in s:
        n = len(t)
        i1, i2 = int(n * s["between"][0]), int(n * s["between"][1])
        q = vc.spline_pose(po, case, (int(t[i1]) + int(t[i2])) // 2)
        probe = (q,) + intr + vc.ALL_TIME
        i1, i2 = _voting_event_at(po, case, probe, Wv, Hv, i1), _voting_event_at(po, case, probe, Wv, Hv, i2)
        grids.append((q,) + intr + (int(t[i1]), int(t[i2])))
        s = dict(s, events=(i1, i2))
    else:
        t0, t1 = int(t[0]), int(t[-1]) + 1
        if "turned" in s:
            q = vc.spline_pose(po, case, t0 + (t1 - t0) // 2)
            for deg in s["turned"]:
                h = math.radians(deg) / 2
                grids.append((vc.q_mul(q, np.array([0.0, math.sin(h), 0.0, math.cos(h)])),) + intr + (t0, t1))
        else:
            edges = [t0 + (t1 - t0) * i // s["slices"] for i in range(s["slices"] + 1)]
            for lo, hi in zip(edges[:-1], edges[1:]):
                grids.append((vc.spline_pose(po, case, lo + (hi - lo) // 2),) + intr + (lo, hi))
    _sets[name] = (case, Wv, Hv, s["bins"], s.get("signed", True), grids)
    if "events" in s:
        _edge_events[name] = s["events"]
    return _sets[name]


_edge_events = {}


def edge_events(po, name):
    """(index of the event whose timestamp is t_lo, index of the event whose timestamp is t_hi) of a `between` set"""
    voxel_set(po, name)
    return _edge_events[name]


def reference_of(po, case, grids, Wv, Hv, n_bins, signed, x, y, t, pol, knots=None, keep=None):
    """(planes[G, n_bins, Hv, Wv] fp32, the same of the votes' ABSOLUTE values, counts[G] int64, near-integer voting events) of ONE
    voxel_add over (x, y, t, pol).  keep: a mask over the events; those outside it are batched and sampled with the rest and do
    not vote (the reference's own identities: the ON events alone, the OFF events alone)."""
    ray, _, sampled = vc.world_rays(po, case, x, y, t, knots)
    t = np.asarray(t, np.int64)
    pol = np.asarray(pol)
    if keep is not None:
        sampled = sampled & keep
    G = len(grids)
    planes = np.zeros((G, n_bins, Hv, Wv), F32)
    absp = np.zeros((G, n_bins, Hv, Wv), F32)
    counts = np.zeros(G, np.int64)
    near = 0
    for k, g in enumerate(grids):
        lo, hi = int(g[5]), int(g[6])
        idx = np.nonzero(sampled & (t >= lo) & (t < hi))[0]
        u, ww, ok = vc.project(g, ray[idx], Wv, Hv)
        idx, u, ww = idx[ok], u[ok], ww[ok]
        counts[k] = len(idx)
        near += int(np.count_nonzero(wc.near_integer(u, ww)))
        xx, yy = np.trunc(u).astype(np.int64), np.trunc(ww).astype(np.int64)
        wb = iwe_numpy._weights((u - xx).astype(F32), (ww - yy).astype(F32))
        if n_bins >= 2:
            scale = float(n_bins - 1) / float(hi - lo)
            tau = (t[idx] - lo).astype(np.float64) * scale
            b0 = np.minimum(np.trunc(tau).astype(np.int64), n_bins - 2)
            f = (tau - b0).astype(F32)
            parts = ((b0, F32(1) - f), (b0 + 1, f))
        else:
            parts = ((np.zeros(len(idx), np.int64), np.ones(len(idx), F32)),)
        s = np.where(pol[idx] != 0, F32(1), F32(-1)).astype(F32) if signed else np.ones(len(idx), F32)
        for b, wt in parts:
            val = (wt[:, None] * wb).astype(F32)
            for bin_ in range(n_bins):
                m = b == bin_
                iwe_numpy._add_votes(planes[k, bin_], yy[m], xx[m], s[m, None] * val[m])
                iwe_numpy._add_votes(absp[k, bin_], yy[m], xx[m], val[m])
    return planes, absp, counts, near


_refs = {}


def reference(po, name):
    """the reference of a set over its configuration's whole stream (computed once, read-only)"""
    if name not in _refs:
        case, Wv, Hv, n_bins, signed, grids = voxel_set(po, name)
        _, x, y, t = rc.window(case)
        out = reference_of(po, case, grids, Wv, Hv, n_bins, signed, x, y, t, pc.polarity(case))
        for a in out[:3]:
            a.setflags(write=False)
        _refs[name] = out
    return _refs[name]


def rel_vox(got, planes, absp):
    """max |got - ref| relative to the largest ABSOLUTE vote sum: an fp32 sum's rounding follows the magnitude of what was added,
    not what remains after ON and OFF cancel"""
    d = np.abs(np.asarray(got, np.float64) - np.asarray(planes, np.float64)).max() if planes.size else 0.0
    return d / max(float(np.abs(absp).max()) if absp.size else 0.0, 1e-30)


def grids_meeting_a_run(po, name):
    """the largest number of grids of a set whose range meets the EVENT times of one vote workgroup's run of packed events
    (cmx_recon.hip: recon_run(per_batch) = min(256 per_batch, 2048) packed events, starting at a multiple of itself)"""
    case, _, _, _, _, grids = voxel_set(po, name)
    c = rc.CASES[case]
    _, x, y, t = rc.window(case)
    B, rate = c["batch"], c["rate"]
    per_batch = (B + rate - 1) // rate
    run = min(256 * per_batch, 2048)
    _, _, sampled = vc.world_rays(po, case, x, y, t)
    ts = np.asarray(t, np.int64)[sampled]
    most = 0
    for e0 in range(0, len(ts), run):
        lo, hi = ts[e0:e0 + run].min(), ts[e0:e0 + run].max()
        most = max(most, sum(1 for g in grids if g[5] <= hi and g[6] > lo))
    return most
