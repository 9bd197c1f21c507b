"""CPU: the header and the Python binding declare the signed polarity panorama, and the numpy reference of its GPU tests
(tests/recon_pol_cases.py) is right before anything is compared with it.  Needs no GPU.

The reference's events with flags == 3 are split by polarity and each half is voted again: the two planes must add up to the
oracle's plane of the configuration, and for every configuration the GPU tests vote, both halves must hold events."""
import os
import re

import numpy as np
import pytest

import recon_cases as rc
import recon_pol_cases as pc
import recon_warp_cases as wc
from util import RTOL, rel_img

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CALLS = ("cmx_events_push_pol", "cmx_events_push_aos_pol", "cmx_events_has_polarity", "cmx_backend_recon_pol_add",
         "cmx_backend_recon_pol_add_aos", "cmx_backend_recon_pol_add_from", "cmx_backend_recon_pol_get", "cmx_backend_recon_pol_render",
         "cmx_backend_recon_pol_reset")


def test_header_and_binding_declare_the_polarity_calls():
    from cmax_slam_amd import _lib, evaluator
    hdr = open(os.path.join(ROOT, "include", "cmax_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in CALLS:
        assert re.search(r"\bint\s+%s\s*\(" % name, code), name
        assert name in _lib.SYMBOLS, name
    assert re.search(r"#define\s+CMX_ABI_VERSION\s+6\b", hdr)  # symbols only: the ABI version stays
    for macro, value in (("CMX_AOS_DVS_POLARITY", 12), ("CMX_POL_MONO8", 0), ("CMX_POL_BGR8", 1)):
        assert re.search(r"#define\s+%s\s+%d\b" % (macro, value), hdr), macro
    assert (_lib.AOS_DVS_POLARITY, _lib.POL_MONO8, _lib.POL_BGR8) == (12, 0, 1)
    assert _lib.DVS_EVENT_DTYPE.fields["polarity"][1] == _lib.AOS_DVS_POLARITY
    # cmx_aos_layout keeps its five fields: it is passed by pointer and its size is ABI
    assert re.search(r"typedef struct \{ size_t stride, off_x, off_y, off_sec, off_nsec; \} cmx_aos_layout;", hdr)
    assert [f[0] for f in _lib.AosLayout._fields_] == ["stride", "off_x", "off_y", "off_sec", "off_nsec"]
    for method in ("reconstruct_pol_add", "reconstruct_pol_add_aos", "reconstruct_pol_add_from", "reconstruct_pol_get",
                   "reconstruct_pol_render", "reconstruct_pol_reset"):
        assert callable(getattr(evaluator.BackendEvaluator, method)), method
    assert isinstance(evaluator.EventStore.has_polarity, property)


@pytest.mark.parametrize("name", pc.USED + pc.EDGE)
def test_the_two_halves_add_up_to_the_oracle_plane(oracle, name):
    c = rc.CASES[name]
    on, off, n_on, n_off = pc.reference(oracle, name)
    px, py, fl = wc.reference(oracle, name)
    assert n_on + n_off == int(np.count_nonzero(fl == 3))
    ref = rc.oracle_plane(oracle, name)
    if c["N"] >= 2:
        r = rel_img(on.astype(np.float64) + off.astype(np.float64), ref)
        print("%s: ON + OFF vs oracle plane %.2e (%d ON, %d OFF events vote)" % (name, r, n_on, n_off))
        assert r < RTOL
    else:
        assert not on.any() and not off.any() and not ref.any()


@pytest.mark.parametrize("name", pc.USED)
def test_both_halves_hold_events(oracle, name):
    on, off, n_on, n_off = pc.reference(oracle, name)
    assert n_on > 0 and n_off > 0 and on.any() and off.any()
    pol = pc.polarity(name)
    assert pol.dtype == np.uint8 and len(pol) == rc.CASES[name]["N"] and set(np.unique(pol)) == {0, 1}
