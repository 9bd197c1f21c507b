"""CPU: the header, the library and the Python binding declare the voxel grids, and the numpy reference of their GPU tests
(tests/recon_voxel_cases.py) is a usable yardstick before anything is compared with it.  Needs no GPU.

Conditions on the inputs: every bin of every grid of every set receives votes (the sets with an edge count n0 / n1 / n2 apart), and
in a signed set votes of both signs.  No set puts more than recon_warp_cases.MAX_NEAR_INTEGER voting events within NEAR_INTEGER of a
cell boundary.  Checks of the reference itself: the bins of an unsigned grid add up to its one-bin form (the two temporal weights of
an event add up to one), a signed volume is the unsigned volume of its ON events less that of its OFF events, and the grid that
starts and ends exactly on an event's timestamp holds the first of the two with tau == 0 and not the second."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import recon_cases as rc
import recon_pol_cases as pc
import recon_view_cases as vc
import recon_voxel_cases as xc
import recon_warp_cases as wc
from util import RTOL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CALLS = ("cmx_backend_recon_voxel_begin", "cmx_backend_recon_voxel_add", "cmx_backend_recon_voxel_add_aos",
         "cmx_backend_recon_voxel_add_from", "cmx_backend_recon_voxel_get", "cmx_backend_recon_voxel_get_device",
         "cmx_backend_recon_voxel_reset", "cmx_backend_recon_voxel_end")


def test_header_library_and_binding_declare_the_voxel_calls():
    from cmax_slam_amd import _lib, evaluator, trajectory
    hdr = open(os.path.join(ROOT, "include", "cmax_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    raw = C.CDLL(_lib.build())
    for name in CALLS:
        assert re.search(r"\bint\s+%s\s*\(" % name, code), name
        assert name in _lib.SYMBOLS, name
        assert hasattr(raw, name), "libcmaxhip.so does not export %s" % name
    assert re.search(r"#define\s+CMX_ABI_VERSION\s+6\b", hdr)  # symbols only: the ABI version stays
    for method in ("reconstruct_voxel_begin", "reconstruct_voxel_add", "reconstruct_voxel_add_aos", "reconstruct_voxel_add_from",
                   "reconstruct_voxel_get", "reconstruct_voxel_reset", "reconstruct_voxel_end"):
        assert callable(getattr(evaluator.BackendEvaluator, method)), method
    assert callable(trajectory.voxel_grids)


def test_voxel_grids_are_frame_views_with_a_finite_range():
    from cmax_slam_amd import trajectory
    c, w = rc.CASES["A"], rc.window("A")[0]
    intr, period = (200.0, 200.0, 119.75, 89.75), 500_000_000
    grids = trajectory.voxel_grids(c["order"], w.knots_true, w.start_ns, w.dt_ns, period, intr)
    views = trajectory.frame_views(c["order"], w.knots_true, w.start_ns, w.dt_ns, period, intr)
    assert len(grids) == len(views) > 3
    for g, v in zip(grids, views):
        assert bytes(g) == bytes(v)
    lo, hi = trajectory.ALL_TIME_NS
    with pytest.raises(ValueError):
        trajectory.voxel_grids(c["order"], w.knots_true, w.start_ns, w.dt_ns, period, intr, t_beg_ns=lo, t_end_ns=hi)
    with pytest.raises(ValueError):
        trajectory.voxel_grids(c["order"], w.knots_true, w.start_ns, w.dt_ns, period, intr, exposure_ns=hi - lo)


@pytest.mark.parametrize("name", list(xc.SETS))
def test_no_set_is_an_empty_comparison(oracle, name):
    case, Wv, Hv, n_bins, signed, grids = xc.voxel_set(oracle, name)
    planes, absp, counts, near = xc.reference(oracle, name)
    assert planes.shape == absp.shape == (len(grids), n_bins, Hv, Wv) and planes.dtype == np.float32
    per_bin = absp.reshape(len(grids), n_bins, -1).sum(axis=2, dtype=np.float64)
    print("%s: votes per grid %s; |votes| per bin %s; %d voting events within %.0e px of a cell boundary" %
          (name, counts.tolist(), np.round(per_bin, 1).tolist(), near, wc.NEAR_INTEGER))
    assert near <= wc.MAX_NEAR_INTEGER
    # four bilinear weights times two temporal weights add up to one per voting event
    assert np.allclose(per_bin.sum(axis=1), counts, rtol=1e-4, atol=1e-3)
    if name in xc.EDGE:
        c = rc.CASES[case]
        assert counts.sum() <= rc.sampled(c["N"], c["batch"], c["rate"])
        return
    assert (counts > 0).all() and (per_bin > 0).all(), (counts, per_bin)
    if signed:
        assert (planes > 0).any(axis=(2, 3)).all() and (planes < 0).any(axis=(2, 3)).all()
    else:
        assert (planes >= 0).all() and np.array_equal(planes, absp)


def test_the_overlapping_set_overflows_a_workgroups_grid_list(oracle):
    src = open(os.path.join(ROOT, "cmax_slam_amd", "csrc", "cmx_internal.hpp")).read()
    chunk = int(re.search(r"constexpr int kReconViewChunk = (\d+);", src).group(1))
    assert xc.grids_meeting_a_run(oracle, "overlap10") == 10 > 3 * chunk and 10 % chunk  # several chunks, the last one partial
    assert xc.grids_meeting_a_run(oracle, "A5") <= 2
    assert xc.grids_meeting_a_run(oracle, "batch5000") == 2  # a run inside ONE batch meets both grids: its events do, its batch time cannot


def test_batch5000_tells_the_event_time_from_the_batch_time(oracle):
    """a batch of 5000 events: its events lie in both grids and in many bins, its batch time in one grid and one pair of bins"""
    case, Wv, Hv, n_bins, signed, grids = xc.voxel_set(oracle, "batch5000")
    _, x, y, t = rc.window(case)
    _, tp, sampled = vc.world_rays(oracle, case, x, y, t)
    t = np.asarray(t, np.int64)
    differs = 0
    for g in grids:
        by_event = sampled & (t >= g[5]) & (t < g[6])
        by_batch = sampled & (tp >= g[5]) & (tp < g[6])
        differs += int(np.count_nonzero(by_event != by_batch))
    assert differs > 1000


@pytest.mark.parametrize("name", ["A5", "B2"])
def test_the_bins_add_up_to_the_one_bin_form(oracle, name):
    case, Wv, Hv, n_bins, _, grids = xc.voxel_set(oracle, name)
    _, x, y, t = rc.window(case)
    pol = pc.polarity(case)
    many = xc.reference_of(oracle, case, grids, Wv, Hv, n_bins, False, x, y, t, pol)
    one = xc.reference_of(oracle, case, grids, Wv, Hv, 1, False, x, y, t, pol)
    assert np.array_equal(many[2], one[2]) and many[3] == one[3]
    total = many[0].sum(axis=1, dtype=np.float64)
    r = np.abs(total - one[0][:, 0]).max() / np.abs(one[0]).max()
    print("%s: %d bins against one, %.2e" % (name, n_bins, r))
    assert r < RTOL


@pytest.mark.parametrize("name", ["A5", "batch5000"])
def test_signed_is_on_less_off(oracle, name):
    case, Wv, Hv, n_bins, _, grids = xc.voxel_set(oracle, name)
    _, x, y, t = rc.window(case)
    pol = pc.polarity(case)
    signed, absp, counts, _ = xc.reference(oracle, name)
    on = xc.reference_of(oracle, case, grids, Wv, Hv, n_bins, False, x, y, t, pol, keep=pol != 0)
    off = xc.reference_of(oracle, case, grids, Wv, Hv, n_bins, False, x, y, t, pol, keep=pol == 0)
    assert np.array_equal(on[2] + off[2], counts) and (on[2] > 0).all() and (off[2] > 0).all()
    r = xc.rel_vox(signed, on[0].astype(np.float64) - off[0].astype(np.float64), absp)
    print("%s: signed against ON - OFF, %.2e" % (name, r))
    assert r < RTOL
    assert xc.rel_vox(absp, on[0].astype(np.float64) + off[0].astype(np.float64), absp) < RTOL


def test_edges_in_time(oracle):
    name = "edges_in_time"
    case, Wv, Hv, n_bins, signed, grids = xc.voxel_set(oracle, name)
    i1, i2 = xc.edge_events(oracle, name)
    _, x, y, t = rc.window(case)
    t = np.asarray(t, np.int64)
    pol = pc.polarity(case)
    (g,) = grids
    assert g[5] == t[i1] and g[6] == t[i2] and 0 < i1 < i2 < len(t) - 1 and t[i1 - 1] < t[i1] and t[i2 - 1] < t[i2]
    planes, absp, counts, _ = xc.reference(oracle, name)
    # every event in [i1, i2) is sampled (rate 1, no lone event among them): the grid's count is those of them inside its plane
    ray, _, sampled = vc.world_rays(oracle, case, x, y, t)
    ok = vc.project(g, ray, Wv, Hv)[2]
    assert sampled[i1:i2 + 1].all() and ok[i1] and ok[i2]
    assert counts[0] == np.count_nonzero(ok[i1:i2]) > 1000
    one = np.zeros(len(t), bool)
    one[i1] = True
    first = xc.reference_of(oracle, case, grids, Wv, Hv, n_bins, signed, x, y, t, pol, keep=one)
    assert first[2][0] == 1 and first[1][0, 0].sum() > 0.999 and not first[1][0, 1:].any()  # tau == 0: all of it in bin 0
    one[:] = False
    one[i2] = True
    second = xc.reference_of(oracle, case, grids, Wv, Hv, n_bins, signed, x, y, t, pol, keep=one)
    assert second[2][0] == 0 and not second[1].any()  # t == t_hi: outside
