"""CPU: the header and the Python binding declare the pinhole views, and the numpy reference of their GPU tests
(tests/recon_view_cases.py) is a usable yardstick before anything is compared with it.  Needs no GPU.

Conditions on the inputs: every view of every set receives at least 100 voting events, except the two turned away from the scene
(by 180 and by 90 degrees: recon_view_cases.SETS says why the second one is empty too), which receive none, and n65, which holds 64
sampled events in all, so that no view of it can reach 100: there the condition is half of them.  No set puts more than
recon_warp_cases.MAX_NEAR_INTEGER voting events within NEAR_INTEGER of a cell boundary; the sets meant to overflow a vote
workgroup's LDS list of views do.  Checks of the reference itself: disjoint slices that cover all
time hold exactly the events the sampling selects, and a camera that does not move sees the events' own pixel histogram."""
import os
import re

import numpy as np
import pytest

import recon_cases as rc
import recon_view_cases as vc
import recon_warp_cases as wc
from util import RTOL, rel_img

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIN_VOTES = 100

CALLS = ("cmx_backend_recon_view_begin", "cmx_backend_recon_view_add", "cmx_backend_recon_view_add_aos",
         "cmx_backend_recon_view_add_from", "cmx_backend_recon_view_get", "cmx_backend_recon_view_render",
         "cmx_backend_recon_view_reset", "cmx_backend_recon_view_end")


def test_header_and_binding_declare_the_view_calls():
    import ctypes as C
    from cmax_slam_amd import _lib, evaluator, trajectory
    hdr = open(os.path.join(ROOT, "include", "cmax_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in CALLS:
        assert re.search(r"\bint\s+%s\s*\(" % name, code), name
        assert name in _lib.SYMBOLS, name
    assert re.search(r"#define\s+CMX_ABI_VERSION\s+6\b", hdr)  # symbols only: the ABI version stays
    assert re.search(r"typedef struct cmx_recon_view \{\s*double\s+quat_xyzw\[4\];\s*double\s+fx, fy, cx, cy;\s*int64_t t_lo_ns, t_hi_ns;\s*\} cmx_recon_view;",
                     code)
    assert [f[0] for f in _lib.ReconView._fields_] == ["quat_xyzw", "fx", "fy", "cx", "cy", "t_lo_ns", "t_hi_ns"]
    assert C.sizeof(_lib.ReconView) == 80
    for method in ("reconstruct_view_begin", "reconstruct_view_add", "reconstruct_view_add_aos", "reconstruct_view_add_from",
                   "reconstruct_view_get", "reconstruct_view_render", "reconstruct_view_reset", "reconstruct_view_end"):
        assert callable(getattr(evaluator.BackendEvaluator, method)), method
    assert callable(trajectory.frame_views) and callable(trajectory.crop_view)


@pytest.mark.parametrize("name", list(vc.SETS))
def test_no_view_is_an_empty_comparison(oracle, name):
    planes, counts, members, near = vc.reference(oracle, name)
    c = rc.CASES[vc.SETS[name]["case"]]
    sampled = rc.sampled(c["N"], c["batch"], c["rate"])
    print("%s: votes per view %s; %d voting events within %.0e px of a cell boundary" % (name, counts.tolist(), near, wc.NEAR_INTEGER))
    for k, n in enumerate(counts):
        if (name, k) in vc.EMPTY_VIEWS:
            assert n == 0 and not planes[k].any()
        else:
            assert n >= min(MIN_VOTES, sampled // 2), (name, k, int(n))
            assert abs(float(planes[k].sum(dtype=np.float64)) - n) < 1e-3 * n  # four weights per event add up to one
    assert near <= wc.MAX_NEAR_INTEGER


def test_the_overlapping_set_overflows_a_workgroups_view_list(oracle):
    src = open(os.path.join(ROOT, "cmax_slam_amd", "csrc", "cmx_internal.hpp")).read()
    chunk = int(re.search(r"constexpr int kReconViewChunk = (\d+);", src).group(1))
    most = vc.views_meeting_a_run(oracle, "overlap40")
    print("overlap40: up to %d views meet one run; a chunk holds %d" % (most, chunk))
    assert most > chunk
    assert vc.views_meeting_a_run(oracle, "stack10") == 10 > 3 * chunk  # several chunks, the last one partial
    assert vc.views_meeting_a_run(oracle, "frames8") <= 2  # the video case: one or two views per run


@pytest.mark.parametrize("name", [n for n, s in vc.SETS.items() if s["slices"] > 0 and "widen" not in s])
def test_disjoint_slices_hold_the_sampled_events(oracle, name):
    c = rc.CASES[vc.SETS[name]["case"]]
    members = vc.reference(oracle, name)[2]
    assert int(members.sum()) == rc.sampled(c["N"], c["batch"], c["rate"]) and (members > 0).all()


@pytest.mark.parametrize("case", ["A", "B"])
def test_a_still_camera_sees_the_pixel_histogram(oracle, case):
    knots, view, want, n_want = vc.still_camera(oracle, case)
    _, x, y, t = rc.window(case)
    planes, counts, _, near = vc.reference_of(oracle, case, [view], vc.W, vc.H, x, y, t, knots=knots)
    r = rel_img(planes[0], want)
    print("%s: still camera %.2e, %d events" % (case, r, n_want))
    assert counts[0] == n_want and n_want > 1000 and near == 0
    assert r < RTOL
