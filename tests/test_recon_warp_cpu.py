"""CPU: the per-event reference of the export tests (tests/recon_warp_cases.py) is right before anything is compared with it, and the
header and the Python binding declare the export.  Needs no GPU.

The reference's events with flags == 3, voted again in event order with the oracle's own vote functions, must give the oracle's
plane of the configuration; its SAMPLED count must be the vote loop's; and at most MAX_NEAR_INTEGER of its events lie within
NEAR_INTEGER of a cell boundary (those may be left out of the GPU tests' cell and flag comparisons)."""
import os
import re

import numpy as np
import pytest

import recon_cases as rc
import recon_warp_cases as wc
from util import RTOL, rel_img

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", wc.ALL)
def test_reference_revoted_is_the_oracle_plane(oracle, name):
    c = rc.CASES[name]
    px, py, fl = wc.reference(oracle, name)
    assert len(px) == len(py) == len(fl) == c["N"]
    assert int(np.count_nonzero(fl & wc.SAMPLED)) == rc.sampled(c["N"], c["batch"], c["rate"])
    plane = wc.revote(px, py, fl, c["Hp"], c["Wp"])
    ref = rc.oracle_plane(oracle, name)
    if c["N"] >= 2:
        r = rel_img(plane, ref)
        print("%s: re-voted reference vs oracle plane %.2e, %d of %d events vote" % (name, r, np.count_nonzero(fl == 3), c["N"]))
        assert r < RTOL
        assert np.count_nonzero(fl == 3) > 0
    else:
        assert not plane.any() and not ref.any()


@pytest.mark.parametrize("name", wc.ALL)
def test_reference_leaves_out_at_most_two_events(oracle, name):
    px, py, _ = wc.reference(oracle, name)
    n_near = int(np.count_nonzero(wc.near_integer(px, py)))
    print("%s: %d events within %g of a cell boundary" % (name, n_near, wc.NEAR_INTEGER))
    assert n_near <= wc.MAX_NEAR_INTEGER


def test_lone_event_and_sampling_rules(oracle):
    # n65: one batch of 64 and a lone event that takes its own time and is not sampled
    _, x, y, t = wc.window("n65")
    tp = wc.pose_times(t, 64)
    assert wc.batches(65, 64) == (1, 64) and wc.batches(64, 64) == (1, -1) and wc.batches(1, 64) == (0, 0) and wc.batches(2, 64) == (1, -1)
    assert tp[64] == t[64] and len(set(tp[:64])) == 1
    fl = wc.reference(oracle, "n65")[2]
    assert not fl[64] & wc.SAMPLED and all(fl[:64] & wc.SAMPLED)
    # batch size 1: every event is a batch of its own at its own time, the last one is the lone one
    _, x, y, t = wc.window("batch1")
    assert np.array_equal(wc.pose_times(t, 1), t)
    fl = wc.reference(oracle, "batch1")[2]
    assert all(fl[:-1] & wc.SAMPLED) and not fl[-1] & wc.SAMPLED
    # B at rate 3: unsampled events carry coordinates
    px, py, fl = wc.reference(oracle, "B")
    assert np.isfinite(px).all() and np.isfinite(py).all()
    assert np.count_nonzero(~(fl & wc.SAMPLED).astype(bool)) == 30_001 - 10_313


def test_header_and_binding_declare_the_export():
    from cmax_slam_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "cmax_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    calls = ("cmx_backend_recon_warp", "cmx_backend_recon_warp_aos", "cmx_backend_recon_warp_from", "cmx_backend_recon_warp_from_device")
    for name in calls:
        assert re.search(r"\bint\s+%s\s*\(" % name, code), name
        assert name in _lib.SYMBOLS
    assert re.search(r"#define\s+CMX_ABI_VERSION\s+6\b", hdr)
    for macro, value in (("CMX_WARP_F64", 0), ("CMX_WARP_F32", 1), ("CMX_WARP_SAMPLED", 1), ("CMX_WARP_INSIDE", 2)):
        assert re.search(r"#define\s+%s\s+%d\b" % (macro, value), hdr), macro
    assert (_lib.WARP_F64, _lib.WARP_F32, _lib.WARP_SAMPLED, _lib.WARP_INSIDE) == (0, 1, 1, 2)
