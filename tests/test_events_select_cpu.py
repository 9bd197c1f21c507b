"""CPU: the event-store selection is declared, bound and exposed (cmx_events_select[_device], _pixel_counts[_device], _read,
cmx_select; EventStore.select / pixel_counts / read) without an ABI bump, the cases of tests/events_select_cases.py are no empty
comparisons, and synth.event_stream's default output is what it was before it learned about hot pixels."""
import ctypes
import hashlib
import os
import re

import numpy as np
import pytest

import events_select_cases as ec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ("cmx_events_select", "cmx_events_select_device", "cmx_events_pixel_counts", "cmx_events_pixel_counts_device", "cmx_events_read")


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cmax_hip.h")).read(), flags=re.S)


def test_header_declares_the_calls_and_the_struct():
    hdr = _header()
    declared = set(re.findall(r"\b(cmx_[a-z0-9_]+)\s*\(", hdr))
    assert set(CALLS) <= declared
    m = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*cmx_select\s*;", hdr)
    assert m, "cmx_select is not declared"
    for member in ("size", "keep", "score", "min_score", "flags", "flags_mask", "flags_value", "pixel_keep"):
        assert re.search(r"\b%s\b" % member, m.group(1)), member


def test_binding_table_has_them():
    from cmax_slam_amd import _lib
    assert set(CALLS) <= set(_lib.SYMBOLS)
    names = [f[0] for f in _lib.Select._fields_]
    assert names == ["size", "keep", "score", "min_score", "flags", "flags_mask", "flags_value", "pixel_keep"]
    # the C layout on an LP64 host: size_t, three pointers, a float and two bytes with their padding
    assert ctypes.sizeof(_lib.Select) == 56 and _lib.Select.flags_mask.offset == 40 and _lib.Select.pixel_keep.offset == 48


def test_event_store_has_the_methods():
    from cmax_slam_amd import evaluator
    for name in ("select", "pixel_counts", "read"):
        assert callable(getattr(evaluator.EventStore, name, None)), name


def test_abi_version_stays_6():
    assert re.search(r"#define\s+CMX_ABI_VERSION\s+6\b", _header())
    assert set(CALLS) <= set(re.findall(r"\b(cmx_[a-z0-9_]+)\s*\(", _header()))  # ... with the calls added


@pytest.mark.parametrize("table,n", [(ec.PATTERNS, ec.N_BIG), (ec.CRITERIA, ec.N_CRIT)], ids=["patterns", "criteria"])
def test_cases_keep_some_and_drop_some(table, n):
    for name in table:
        kind, sel, keep = ec.kept_of_case(table, name, n)
        assert keep.dtype == np.bool_ and keep.shape == (n,)
        if kind == "all":
            assert keep.all(), name
        elif kind == "none":
            assert not keep.any(), name
        else:
            assert kind == "some" and keep.any() and not keep.all(), name
    assert n > ec.TILE and n % 64 != 0 and n % ec.TILE != 0


def test_counts_reach_every_edge():
    for edge in (64, 256, ec.TILE, ec.TILE_MAX):
        assert {edge - 1, edge, edge + 1} <= set(ec.COUNTS)
    assert {0, 1, ec.N_BIG} <= set(ec.COUNTS) and ec.N_BIG == 3 * 8192 + 17
    assert ec.N_SCAN == ec.SCAN_PASS * ec.TILE + 1
    assert ec.N_BASE >= ec.N_BIG + 67


def test_special_scores_are_there():
    s = ec.scores(ec.N_CRIT)
    assert np.isnan(s).sum() >= 3 and np.isposinf(s).any() and np.isneginf(s).any()
    assert ((s == 0) & np.signbit(s)).any() and (s == np.float32(0.25)).any()
    k = ec.predicate(dict(score=s, min_score=-np.inf), np.zeros(len(s), int), np.zeros(len(s), int), ec.W)
    assert (k == ~np.isnan(s)).all()
    k0 = ec.predicate(dict(score=ec.scores(ec.N_CRIT, 5, 0.0), min_score=0.0), np.zeros(len(s), int), np.zeros(len(s), int), ec.W)
    s0 = ec.scores(ec.N_CRIT, 5, 0.0)
    assert k0[(s0 == 0) & np.signbit(s0)].all()  # -0.0 >= 0.0


def test_base_stream_and_hot_pixels():
    x, y, t, pol, is_hot, hot_xy = ec.stream()
    assert len(x) == ec.N_BASE and (np.diff(t) >= 0).all() and set(np.unique(pol)) == {0, 1}
    assert hot_xy.shape == (2, 2) and tuple(hot_xy[0]) != tuple(hot_xy[1])
    assert is_hot.sum() == round(ec.N_BASE * ec.HOT_SHARE)
    at_hot = ((x == hot_xy[0, 0]) & (y == hot_xy[0, 1])) | ((x == hot_xy[1, 0]) & (y == hot_xy[1, 1]))
    assert (at_hot[is_hot]).all()
    keep = ec.predicate(dict(pixel_keep=ec.hot_mask()), x, y, ec.W)
    assert (keep == ~at_hot).all() and int((~keep).sum()) >= int(is_hot.sum())
    cx, cy, ct, cp = ec.compact((x, y, t, pol), keep)
    assert len(cx) == keep.sum() and (np.diff(ct) >= 0).all() and ec.compact((None,), keep) == (None,)


def _digest(s):
    return hashlib.sha256(s.x.tobytes() + s.y.tobytes() + s.t_ns.tobytes() + s.grid_quat.tobytes() + s.grid_omega.tobytes()).hexdigest()


def test_default_event_stream_is_unchanged():
    """byte-identical with and without the new keyword arguments at their defaults, and identical with the output recorded before the
    arguments existed (sha256 over x, y, t_ns, grid_quat, grid_omega of this call)"""
    from cmax_slam_amd import synth
    args = (200000, 0.2, 240, 180, 200.0, 200.0, 119.5, 89.5)
    a = synth.event_stream(*args, seed=3)
    b = synth.event_stream(*args, seed=3, hot_pixels=0, hot_share=0.0)
    c = synth.event_stream(*args, seed=3, hot_pixels=0, hot_share=0.5)  # no pixels: no share either
    assert _digest(a) == _digest(b) == _digest(c) == "c072929cd14f4eb82df7dd366fd2b27840ea66ecf23a74eb7eb331b39cc88aae"
    assert a.x.dtype == np.uint16 and a.t_ns.dtype == np.int64 and not a.is_hot.any() and len(a.is_hot) == len(a.x)
    h = synth.event_stream(*args, seed=3, hot_pixels=2, hot_share=0.04)
    assert len(h.x) == len(a.x) and h.is_hot.sum() == round(0.04 * len(a.x)) and (np.diff(h.t_ns) >= 0).all()
