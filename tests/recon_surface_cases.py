"""The reference of the time-surface tests (tests/test_gpu_recon_surface.py): the latest timestamp per pixel and polarity of a set of
surfaces over a recon_cases configuration, in numpy, built from pieces the suite already trusts -- recon_view_cases.world_rays for
batch membership, batch pose and world ray, recon_view_cases.project for the view's projection and vote test,
recon_pol_cases.polarity for the events' polarity, recon_warp_cases.near_integer for the events a rounding may move to the
neighbouring cell -- with the per-event rules of include/cmax_hip.h:

  an event belongs to every surface with t_lo <= t_i < t_hi, t_i its OWN timestamp;  cx = trunc(u + 0.5), cy = trunc(w + 0.5);
  channel 1 for an OFF event of a by-polarity set, else channel 0;  cell = max(cell, t_i) as int64;  an empty cell holds -2**63.

A maximum of integers has no rounding: the GPU cells are compared with these EXACTLY, except at the two cells an event within
recon_warp_cases.NEAR_INTEGER of a half-pixel boundary may choose between.  tests/test_recon_surface_cpu.py counts those events
(none, and never more than MAX_NEAR_INTEGER), checks that no set is an empty comparison, and that the reference holds its own
identities.

Sets: the twelve geometries of recon_voxel_cases.SETS through recon_voxel_cases.voxel_set, read-only and by polarity (one_bin is
merged, as it is unsigned there), and all_time: configuration A, one 96 x 64 view over trajectory.ALL_TIME_NS along the spline's
pose at mid-stream -- the range the voxel grids refuse and a surface accepts."""
import numpy as np

import recon_cases as rc
import recon_pol_cases as pc
import recon_view_cases as vc
import recon_voxel_cases as xc
import recon_warp_cases as wc

EMPTY = -2 ** 63

SETS = tuple(xc.SETS) + ("all_time",)
EDGE = xc.EDGE  # sets whose surface may stay empty

_sets = {}


def surface_set(po, name):
    """(configuration, Wv, Hv, by_polarity, [(quat_xyzw, fx, fy, cx, cy, t_lo_ns, t_hi_ns), ...]) of a set: built once"""
    if name not in _sets:
        if name == "all_time":
            from cmax_slam_amd import trajectory
            case, Wv, Hv = "A", 96, 64
            _, _, _, t = rc.window(case)
            q = vc.spline_pose(po, case, (int(t[0]) + int(t[-1])) // 2)
            _sets[name] = (case, Wv, Hv, True, [(q,) + vc.scaled_intrinsics(Wv, Hv) + tuple(trajectory.ALL_TIME_NS)])
        else:
            case, Wv, Hv, _, signed, grids = xc.voxel_set(po, name)
            _sets[name] = (case, Wv, Hv, bool(signed), list(grids))
    return _sets[name]


def reference_of(po, case, surfaces, Wv, Hv, by_polarity, x, y, t, pol, knots=None, keep=None, last_wins=False):
    """(cells[S, C, Hv, Wv] int64, counts[S] int64, near-boundary voting events, votes per cell [S, C, Hv, Wv] int64,
    distinct[S, C, Hv, Wv] bool: the cell received two or more different timestamps) of ONE surface_add over (x, y, t, pol).
    keep: a mask over the events; those outside it are batched and sampled with the rest and do not vote.
    last_wins: the cells are written in event order, a plain store -- the same as the maximum for a time-sorted stream."""
    ray, _, sampled = vc.world_rays(po, case, x, y, t, knots)
    t = np.asarray(t, np.int64)
    pol = np.asarray(pol)
    if keep is not None:
        sampled = sampled & keep
    S, C = len(surfaces), 2 if by_polarity else 1
    cells = np.full((S, C, Hv, Wv), EMPTY, np.int64)
    lowest = np.full((S, C, Hv, Wv), 2 ** 63 - 1, np.int64)
    votes = np.zeros((S, C, Hv, Wv), np.int64)
    counts = np.zeros(S, np.int64)
    near = 0
    for k, g in enumerate(surfaces):
        lo, hi = int(g[5]), int(g[6])
        idx = np.nonzero(sampled & (t >= lo) & (t < hi))[0]
        u, ww, ok = vc.project(g, ray[idx], Wv, Hv)
        idx, u, ww = idx[ok], u[ok], ww[ok]
        counts[k] = len(idx)
        near += int(np.count_nonzero(wc.near_integer(u + 0.5, ww + 0.5)))
        cx, cy = np.trunc(u + 0.5).astype(np.int64), np.trunc(ww + 0.5).astype(np.int64)
        ch = np.where(pol[idx] != 0, 0, 1) if by_polarity else np.zeros(len(idx), np.int64)
        if last_wins:
            for c_, y_, x_, t_ in zip(ch, cy, cx, t[idx]):  # (in event order)
                cells[k, c_, y_, x_] = t_
        else:
            np.maximum.at(cells[k], (ch, cy, cx), t[idx])
        np.minimum.at(lowest[k], (ch, cy, cx), t[idx])
        np.add.at(votes[k], (ch, cy, cx), 1)
    return cells, counts, near, votes, (votes >= 2) & (lowest < cells)


_refs = {}


def reference(po, name):
    """the reference of a set over its configuration's whole stream (computed once, read-only)"""
    if name not in _refs:
        case, Wv, Hv, by_pol, surfaces = surface_set(po, name)
        _, x, y, t = rc.window(case)
        out = reference_of(po, case, surfaces, Wv, Hv, by_pol, x, y, t, pc.polarity(case))
        for a in (out[0], out[1], out[3], out[4]):
            a.setflags(write=False)
        _refs[name] = out
    return _refs[name]


def decay_reference(cells, t_ref, tau_ns):
    """the header's decay of int64 cells [S, ...] with one reference time per surface: fp64 quotient and exp, one rounding to fp32"""
    cells = np.asarray(cells, np.int64)
    ref = np.asarray(t_ref, np.int64).reshape((-1,) + (1,) * (cells.ndim - 1))
    empty, late = cells == EMPTY, cells >= ref
    d = np.where(empty | late, np.uint64(0), ref.astype(np.uint64) - cells.astype(np.uint64)).astype(np.float64)  # (modulo 2^64: exact)
    out = np.exp(-(d / float(tau_ns))).astype(np.float32)
    out[late] = 1.0
    out[empty] = 0.0
    return out
