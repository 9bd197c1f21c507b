"""CPU: the header, the library and the Python binding declare the time surfaces, and the numpy reference of their GPU tests
(tests/recon_surface_cases.py) is a usable yardstick before anything is compared with it.  Needs no GPU.

Conditions on the inputs: no set puts more than recon_warp_cases.MAX_NEAR_INTEGER voting events within NEAR_INTEGER of a half-pixel
boundary (the cap is not to be raised: a set that breaks it gets another orientation); in every set but n0 / n1 / n2 each surface has
cells that received two or more events with DIFFERENT timestamps, so a kernel that kept the first, or any, vote would not pass; in a
by-polarity set both channels are reached.  Checks of the reference itself: maximum(ON, OFF) is the merged surface of the same views,
for a time-sorted stream the maximum is "the last event written wins", and the surface that starts and ends exactly on an event's
timestamp holds the first of the two and never the second."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import recon_cases as rc
import recon_pol_cases as pc
import recon_surface_cases as sc
import recon_view_cases as vc
import recon_voxel_cases as xc
import recon_warp_cases as wc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CALLS = ("cmx_backend_recon_surface_begin", "cmx_backend_recon_surface_add", "cmx_backend_recon_surface_add_aos",
         "cmx_backend_recon_surface_add_from", "cmx_backend_recon_surface_get", "cmx_backend_recon_surface_get_device",
         "cmx_backend_recon_surface_decay", "cmx_backend_recon_surface_decay_device", "cmx_backend_recon_surface_reset",
         "cmx_backend_recon_surface_end")


def test_header_library_and_binding_declare_the_surface_calls():
    from cmax_slam_amd import _lib, evaluator, trajectory
    hdr = open(os.path.join(ROOT, "include", "cmax_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    raw = C.CDLL(_lib.build())
    assert len(CALLS) == 10
    for name in CALLS:
        assert re.search(r"\bint\s+%s\s*\(" % name, code), name
        assert name in _lib.SYMBOLS, name
        assert hasattr(raw, name), "libcmaxhip.so does not export %s" % name
    assert code.index("cmx_backend_recon_surface_begin") > code.index("cmx_backend_recon_voxel_end")  # after the voxel block
    assert re.search(r"#define\s+CMX_ABI_VERSION\s+6\b", hdr)  # symbols only: the ABI version stays
    for method in ("reconstruct_surface_begin", "reconstruct_surface_add", "reconstruct_surface_add_aos", "reconstruct_surface_add_from",
                   "reconstruct_surface_get", "reconstruct_surface_decay", "reconstruct_surface_reset", "reconstruct_surface_end"):
        assert callable(getattr(evaluator.BackendEvaluator, method)), method
    assert trajectory.SURFACE_EMPTY == -2 ** 63 == sc.EMPTY == np.iinfo(np.int64).min


def test_the_sets_are_the_voxel_geometries_and_all_time(oracle):
    from cmax_slam_amd import trajectory
    assert len(xc.SETS) == 12 and sc.SETS == tuple(xc.SETS) + ("all_time",)
    for name in xc.SETS:
        case, Wv, Hv, by_pol, surfaces = sc.surface_set(oracle, name)
        vcase, vWv, vHv, _, signed, grids = xc.voxel_set(oracle, name)
        assert (case, Wv, Hv, by_pol) == (vcase, vWv, vHv, signed) and len(surfaces) == len(grids)
        assert by_pol == (name != "one_bin")
    case, Wv, Hv, by_pol, (s,) = sc.surface_set(oracle, "all_time")
    assert (case, Wv, Hv, by_pol) == ("A", 96, 64, True) and (s[5], s[6]) == tuple(trajectory.ALL_TIME_NS) == vc.ALL_TIME


@pytest.mark.parametrize("name", sc.SETS)
def test_no_set_is_an_empty_comparison(oracle, name):
    case, Wv, Hv, by_pol, surfaces = sc.surface_set(oracle, name)
    cells, counts, near, votes, distinct = sc.reference(oracle, name)
    S, C_ = len(surfaces), 2 if by_pol else 1
    assert cells.shape == votes.shape == distinct.shape == (S, C_, Hv, Wv) and cells.dtype == np.int64
    reached = cells != sc.EMPTY
    print("%s: votes per surface %s into %s cells, %s of them with two or more different timestamps; %d voting events within %.0e px "
          "of a half-pixel boundary" % (name, counts.tolist(), reached.sum(axis=(1, 2, 3)).tolist(),
                                        distinct.sum(axis=(1, 2, 3)).tolist(), near, wc.NEAR_INTEGER))
    assert near <= wc.MAX_NEAR_INTEGER
    assert np.array_equal(votes.sum(axis=(1, 2, 3)), counts) and np.array_equal(reached, votes > 0)
    # the vote test keeps the border cells empty: 1 <= u < Wv - 2 puts the nearest pixel into [1, Wv - 2]
    assert not reached[..., 0].any() and not reached[..., Wv - 1].any() and not reached[:, :, 0].any() and not reached[:, :, Hv - 1].any()
    _, _, _, t = rc.window(case)
    for k, g in enumerate(surfaces):  # every timestamp lies inside the surface's range
        assert (cells[k][reached[k]] >= g[5]).all() and (cells[k][reached[k]] < g[6]).all()
    if name in sc.EDGE:
        c = rc.CASES[case]
        assert counts.sum() <= rc.sampled(c["N"], c["batch"], c["rate"])
        return
    assert (counts > 0).all()
    assert distinct.any(axis=(1, 2, 3)).all(), "a surface without a cell that saw two different timestamps"
    if by_pol:
        assert reached.any(axis=(2, 3)).all(), "a channel no event reached"


def test_maximum_of_the_channels_is_the_merged_surface(oracle):
    for name in ("A5", "batch5000"):
        case, Wv, Hv, by_pol, surfaces = sc.surface_set(oracle, name)
        assert by_pol
        _, x, y, t = rc.window(case)
        pol = pc.polarity(case)
        cells, counts, _, _, _ = sc.reference(oracle, name)
        merged = sc.reference_of(oracle, case, surfaces, Wv, Hv, False, x, y, t, pol)
        assert merged[0].shape == (len(surfaces), 1, Hv, Wv) and np.array_equal(merged[1], counts)
        assert np.array_equal(np.maximum(cells[:, 0], cells[:, 1]), merged[0][:, 0])
        # ... and each channel is the surface of its own events alone
        on = sc.reference_of(oracle, case, surfaces, Wv, Hv, False, x, y, t, pol, keep=pol != 0)
        off = sc.reference_of(oracle, case, surfaces, Wv, Hv, False, x, y, t, pol, keep=pol == 0)
        assert np.array_equal(on[0][:, 0], cells[:, 0]) and np.array_equal(off[0][:, 0], cells[:, 1])
        assert np.array_equal(on[1] + off[1], counts) and (on[1] > 0).all() and (off[1] > 0).all()


@pytest.mark.parametrize("name", ["A5", "B2", "overlap10"])
def test_for_a_sorted_stream_the_last_event_written_wins(oracle, name):
    case, Wv, Hv, by_pol, surfaces = sc.surface_set(oracle, name)
    _, x, y, t = rc.window(case)
    assert (np.diff(np.asarray(t, np.int64)) >= 0).all()
    cells, counts, _, _, _ = sc.reference(oracle, name)
    last = sc.reference_of(oracle, case, surfaces, Wv, Hv, by_pol, x, y, t, pc.polarity(case), last_wins=True)
    assert np.array_equal(last[0], cells) and np.array_equal(last[1], counts)


def test_edges_in_time(oracle):
    name = "edges_in_time"
    case, Wv, Hv, by_pol, surfaces = sc.surface_set(oracle, name)
    i1, i2 = xc.edge_events(oracle, name)
    _, x, y, t = rc.window(case)
    t = np.asarray(t, np.int64)
    pol = pc.polarity(case)
    (g,) = surfaces
    assert g[5] == t[i1] and g[6] == t[i2] and t[i1 - 1] < t[i1] and t[i2 - 1] < t[i2]
    cells, counts, _, _, _ = sc.reference(oracle, name)
    one = np.zeros(len(t), bool)
    one[i1] = True
    first = sc.reference_of(oracle, case, surfaces, Wv, Hv, by_pol, x, y, t, pol, keep=one)
    assert first[1][0] == 1 and np.count_nonzero(first[0] != sc.EMPTY) == 1 and first[0].max() == t[i1] == g[5]
    assert (cells[first[0] != sc.EMPTY] >= t[i1]).all()  # that cell of the whole reference holds it or a later event
    one[:] = False
    one[i2] = True
    second = sc.reference_of(oracle, case, surfaces, Wv, Hv, by_pol, x, y, t, pol, keep=one)
    assert second[1][0] == 0 and (second[0] == sc.EMPTY).all()  # t == t_hi: outside
    assert cells.max() < t[i2] and cells[cells != sc.EMPTY].min() >= t[i1]


def test_decay_reference():
    cells = np.array([[sc.EMPTY, 100, 1000, 1500, -2 ** 62]], np.int64)
    out = sc.decay_reference(cells, [1000], 300.0)
    assert out.dtype == np.float32 and out[0, 0] == 0.0 and out[0, 2] == 1.0 and out[0, 3] == 1.0
    assert out[0, 1] == np.float32(np.exp(-3.0)) and out[0, 4] == 0.0  # (exp(-1.5e16) underflows to zero)
    wide = sc.decay_reference(np.array([[-2 ** 62]], np.int64), [2 ** 62], float(2 ** 63))  # the difference does not fit an int64
    assert wide[0, 0] == np.float32(np.exp(-1.0))
