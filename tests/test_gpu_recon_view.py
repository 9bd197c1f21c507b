"""GPU: pinhole views of a reconstruction (cmx_backend_recon_view_* / BackendEvaluator.reconstruct_view_*): motion-compensated
event frames and zoomed crops voted on the device, against the numpy reference of tests/recon_view_cases.py.

Bounds.  Default mode: RTOL of tests/util.py on rel_img, the bound every fp32-atomic plane of this suite is held to against its
numpy reference (the planes differ by summation order, and by the fused multiply-adds of be_rotate in the ray: ~1e-16 relative in a
coordinate, far below an fp32 weight's rounding); every counter exactly -- tests/test_recon_view_cpu.py has checked that no voting
event of any set lies within 1e-9 px of a cell boundary.  Deterministic mode: a plane is a sum of integers, so run to run, ingest
path to ingest path, slice to slice, cut to cut and view set to view set it is compared bit for bit.  Render: the rule of
tests/display_ref.py (exact wherever the level is decided, one grey level where the two pow functions may differ), and equality
with cmx_backend_render_map's image of the same plane, the bound tests/test_gpu_recon.py holds recon_render to."""
import os
import sys

import numpy as np
import pytest

import display_ref
import recon_cases as rc
import recon_view_cases as vc
from cmax_slam_amd import _lib, synth, trajectory
from util import RTOL, rel_img

pytestmark = pytest.mark.gpu
W, H = rc.SENSOR[:2]


def make(hip, case, deterministic=False):
    c, w = rc.CASES[case], rc.window(case)[0]
    be = hip.BackendEvaluator(W, H, w.lut, c["Wp"], c["Hp"])
    if deterministic:
        be.set_deterministic(True)
    return be


def begin(be, case, knots=None):
    c, w = rc.CASES[case], rc.window(case)[0]
    be.reconstruct_begin(c["order"], w.knots_true if knots is None else knots, w.start_ns, w.dt_ns, c["batch"], c["rate"])


def store_of(hip, case):
    _, x, y, t = rc.window(case)
    store = hip.EventStore(W, H, max(len(x), 1))
    if len(x):
        store.push(x, y, t)
    return store


def status_of(hip, fn, *a, **k):
    with pytest.raises(hip.CmaxHipError) as e:
        fn(*a, **k)
    return e.value.status


def same(a, b):
    """two results of reconstruct_view_get(with_counts=True), bit for bit"""
    return a[0].shape == b[0].shape and a[0].tobytes() == b[0].tobytes() and np.array_equal(a[1], b[1])


def got(be):
    return be.reconstruct_view_get(with_counts=True)


def voted(hip, oracle, name, deterministic=True, only=None):
    """reconstruct_view_get(with_counts=True) after one view_add_from of the set (or of its views `only`) over the whole stream"""
    case, Wv, Hv, views = vc.view_set(oracle, name)
    be, store = make(hip, case, deterministic), store_of(hip, case)
    begin(be, case)
    be.reconstruct_view_begin(views if only is None else [views[k] for k in only], Wv, Hv)
    be.reconstruct_view_add_from(store, 0, rc.CASES[case]["N"])
    out = got(be)
    be.reconstruct_view_end()
    be.reconstruct_end()
    store.close()
    return out


# ---------------------------------------------------------------- 1. / 4. against the reference, default mode
@pytest.mark.parametrize("name", list(vc.SETS))
def test_default_mode_against_the_numpy_reference(hip, oracle, name):
    ref_planes, ref_counts, _, _ = vc.reference(oracle, name)
    planes, counts = voted(hip, oracle, name, deterministic=False)
    assert planes.shape == ref_planes.shape
    worst = 0.0
    for k in range(len(ref_counts)):
        if (name, k) in vc.EMPTY_VIEWS:
            assert counts[k] == 0 and not planes[k].any(), k
        else:
            worst = max(worst, rel_img(planes[k], ref_planes[k]))
    print("%s: %d views, worst plane %.2e against the reference; votes %s (reference %s)" %
          (name, len(counts), worst, counts.tolist(), ref_counts.tolist()))
    assert worst < RTOL
    assert np.array_equal(counts, ref_counts)


# ---------------------------------------------------------------- 2. deterministic mode, bitwise
@pytest.mark.parametrize("name", ["frames8", "overlap40", "linear", "n65"])
def test_deterministic_mode_is_bitwise(hip, oracle, name):
    case, Wv, Hv, views = vc.view_set(oracle, name)
    c = rc.CASES[case]
    _, x, y, t = rc.window(case)
    n, B = c["N"], c["batch"]
    want = voted(hip, oracle, name)
    ref_planes, ref_counts, _, _ = vc.reference(oracle, name)
    assert np.array_equal(want[1], ref_counts) and max(rel_img(want[0][k], ref_planes[k]) for k in range(len(views))) < RTOL
    assert same(voted(hip, oracle, name), want)  # run to run
    be, store = make(hip, case, True), store_of(hip, case)
    begin(be, case)
    be.reconstruct_view_begin(views, Wv, Hv)
    records = _lib.dvs_events(x, y, t)
    paths = ((be.reconstruct_view_add_from, (store, 0, n)), (be.reconstruct_view_add, (x, y, t)), (be.reconstruct_view_add_aos, (records,)))
    L = _lib.lib()
    try:
        for n_slice in (0, 2 * B, 4096):  # the default (one slice); two batches per slice; a few slices
            assert L.cmx_diag_set(_lib.DIAG_RECON_SLICE_EVENTS, n_slice) == 0
            for fn, args in paths:
                be.reconstruct_view_reset()
                fn(*args)
                assert same(got(be), want), (n_slice, fn.__name__)
    finally:
        assert L.cmx_diag_set(_lib.DIAG_RECON_SLICE_EVENTS, 0) == 0
    if n > 40 * B:  # add(A); add(B) cut at a batch multiple against add(A || B)
        cut = 37 * B
        be.reconstruct_view_reset()
        be.reconstruct_view_add_from(store, 0, cut)
        be.reconstruct_view_add_from(store, cut, n - cut)
        assert same(got(be), want)
        be.reconstruct_view_reset()
        be.reconstruct_view_add(x[:cut], y[:cut], t[:cut])
        be.reconstruct_view_add_aos(records[cut:])
        assert same(got(be), want)
    # a sub-range of the set through get
    part = be.reconstruct_view_get(1, len(views) - 1, with_counts=True) if len(views) > 1 else None
    if part is not None:
        assert part[0].tobytes() == want[0][1:].tobytes() and np.array_equal(part[1], want[1][1:])
    be.reconstruct_end()
    store.close()


@pytest.mark.parametrize("name", ["overlap40", "stack10"])
def test_a_view_does_not_depend_on_the_rest_of_the_set(hip, oracle, name):
    """the chunked list: more views meet a run than a workgroup holds in LDS at a time"""
    n_views = len(vc.view_set(oracle, name)[3])
    among = voted(hip, oracle, name)
    for j in (0, n_views // 2, n_views - 1):
        alone = voted(hip, oracle, name, only=[j])
        assert alone[1][0] > 0
        assert alone[0][0].tobytes() == among[0][j].tobytes() and alone[1][0] == among[1][j], j
    # ... nor on the order the views are given in
    order = list(range(n_views))[::-1]
    back = voted(hip, oracle, name, only=order)
    assert back[0][::-1].tobytes() == among[0].tobytes() and np.array_equal(back[1][::-1], among[1])


# ---------------------------------------------------------------- 3. still camera
@pytest.mark.parametrize("deterministic", [False, True])
def test_a_still_camera_sees_the_pixel_histogram(hip, oracle, deterministic):
    case = "A"
    knots, view, want, n_want = vc.still_camera(oracle, case)
    _, x, y, t = rc.window(case)
    be = make(hip, case, deterministic)
    begin(be, case, knots)
    be.reconstruct_view_begin([view], W, H)
    be.reconstruct_view_add(x, y, t)
    planes, counts = got(be)
    be.reconstruct_end()
    r = rel_img(planes[0], want)
    print("still camera: %.2e against the spread histogram, %d events" % (r, counts[0]))
    assert counts[0] == n_want
    assert r < RTOL


# ---------------------------------------------------------------- 5. edge counts
@pytest.mark.parametrize("case", vc.EDGE)
def test_edge_counts(hip, oracle, case):
    """n0 and n1: no batch, nothing votes.  n2 is one batch of two events in add*'s vote loop (recon_cases.sampled(2, 64, 1) == 2),
    so here too both are warped, and they vote where the reference says -- once per call."""
    _, x, y, t = rc.window(case)
    views = vc.edge_views(oracle, case)
    ref_planes, ref_counts, members, _ = vc.reference_of(oracle, case, views, 96, 64, x, y, t)
    assert members.tolist() == [rc.sampled(len(x), rc.CASES[case]["batch"], rc.CASES[case]["rate"])] == [2 if case == "n2" else 0]
    be, store = make(hip, case, True), store_of(hip, case)
    begin(be, case)
    be.reconstruct_view_begin(views, 96, 64)
    be.reconstruct_view_add(x, y, t)
    be.reconstruct_view_add_aos(_lib.dvs_events(x, y, t))
    be.reconstruct_view_add_from(store, 0, len(x))
    planes, counts = got(be)
    assert planes.shape == (1, 64, 96) and counts.tolist() == [3 * ref_counts[0]]
    if ref_counts[0] == 0:
        assert not planes.any() and (be.reconstruct_view_render(0) == 255).all()
    else:
        assert rel_img(planes[0], 3.0 * ref_planes[0].astype(np.float64)) < RTOL
    be.reconstruct_view_end()
    be.reconstruct_end()
    store.close()


# ---------------------------------------------------------------- 6. nothing else moves
def test_the_view_calls_change_nothing_else(hip, oracle):
    case = "window"
    c, (w, x, y, t) = rc.CASES[case], rc.window(case)
    n = c["N"]
    views = [(np.array(w.knots_true[3]),) + vc.scaled_intrinsics(96, 64) + vc.ALL_TIME,
             (np.array(w.knots_true[6]),) + vc.scaled_intrinsics(96, 64) + (int(t[n // 3]), int(t[2 * n // 3]))]
    ref_planes, ref_counts, _, _ = vc.reference_of(oracle, case, views, 96, 64, x, y, t)
    assert (ref_counts >= 100).all()
    be, store = make(hip, case, True), store_of(hip, case)
    pol = np.random.default_rng(3).integers(0, 2, n).astype(np.uint8)

    def view_calls():
        be.reconstruct_view_begin(views, 96, 64)
        be.reconstruct_view_add_from(store, 0, n)
        out = got(be)
        be.reconstruct_view_render(1)
        be.reconstruct_view_end()
        assert np.array_equal(out[1], ref_counts) and max(rel_img(out[0][k], ref_planes[k]) for k in range(2)) < RTOL
        return out

    def state():
        plane = be.reconstruct_get(with_counts=True)
        pols = be.reconstruct_pol_get(with_counts=True)
        return (plane[0].tobytes(), plane[1:], pols[0].tobytes(), pols[1].tobytes(), pols[2:])

    begin(be, case)
    be.reconstruct_add_from(store, 0, n)
    be.reconstruct_pol_add(x, y, t, pol)
    be.reconstruct_contrast(1.0, want_grad=True)
    be.reconstruct_grad_add_from(store, 0, 10_000)
    before = state()
    once = view_calls()
    be.reconstruct_grad_add_from(store, 10_000, n - 10_000)
    grad = be.reconstruct_grad_get()  # (CMX_ERR_STATE had a view call closed the pass or touched its counts)
    assert np.abs(grad).max() > 0 and state() == before
    ref = make(hip, case, True)
    begin(ref, case)
    ref.reconstruct_add_from(store, 0, n)
    ref.reconstruct_contrast(1.0, want_grad=True)
    ref.reconstruct_grad_add_from(store, 0, 10_000)  # (the same cuts: the gradient sums are bitwise per sequence of calls)
    ref.reconstruct_grad_add_from(store, 10_000, n - 10_000)
    assert ref.reconstruct_grad_get().tobytes() == grad.tobytes()
    # a binding, without and with a frozen head, and after release_head
    ref.reconstruct_bind(store, 0, n)
    be.reconstruct_bind(store, 0, n)
    for step in ("bound", "frozen", "released"):
        for e in (be, ref):
            if step == "frozen":
                e.reconstruct_freeze_head(5)
            if step == "released":
                e.reconstruct_release_head()
        ev = be.reconstruct_eval_bound(None, 1.0)
        infos = (be.reconstruct_bound_info(), be.reconstruct_frozen_info(), be.reconstruct_online_info())
        before = state()
        assert same(view_calls(), once), step
        assert state() == before
        assert (be.reconstruct_bound_info(), be.reconstruct_frozen_info(), be.reconstruct_online_info()) == infos
        ev2, ev_ref = be.reconstruct_eval_bound(None, 1.0), ref.reconstruct_eval_bound(None, 1.0)
        assert ev2[0] == ev[0] == ev_ref[0] and ev2[1].tobytes() == ev[1].tobytes() == ev_ref[1].tobytes(), step
        if step == "released":
            assert infos[2]["released_sampled"] > 0
    ref.reconstruct_end()
    be.reconstruct_end()
    store.close()


# ---------------------------------------------------------------- 7. lifecycle
def test_lifecycle(hip, oracle):
    name = "frames8"
    case, Wv, Hv, views = vc.view_set(oracle, name)
    c, (w, x, y, t) = rc.CASES[case], rc.window(case)
    n = c["N"]
    want = voted(hip, oracle, name)
    be, store = make(hip, case, True), store_of(hip, case)
    begin(be, case)
    assert be.reconstruct_view_end() is None  # view_end without view_begin is not an error
    be.reconstruct_view_begin(views, Wv, Hv)
    zero = got(be)
    assert zero[0].shape == (8, Hv, Wv) and not zero[0].any() and not zero[1].any()

    def cleared():
        p, cnt = got(be)
        return not p.any() and not cnt.any()

    be.reconstruct_view_add_from(store, 0, n)
    assert same(got(be), want)
    be.reconstruct_view_add_from(store, 0, n)  # accumulation goes on after a get
    twice = got(be)
    assert np.array_equal(twice[1], 2 * want[1])
    be.reconstruct_view_reset()
    assert cleared()
    be.reconstruct_view_add_from(store, 0, n)
    assert same(got(be), want)
    # extend and eval_bound move knots or planes of the reconstruction and leave the view planes alone
    be.reconstruct_bind(store, 0, n)
    be.reconstruct_eval_bound(None, 1.0, want_grad=False)
    assert same(got(be), want)
    be.reconstruct_unbind()
    grown = np.vstack([w.knots_true, w.knots_true[-1:]])
    be.reconstruct_extend(grown)
    assert same(got(be), want)
    be.reconstruct_view_reset()
    be.reconstruct_view_add_from(store, 0, n)   # (the first K knots are the old ones: the same poses)
    assert same(got(be), want)
    # restart clears and keeps the views
    be.reconstruct_restart(grown)
    assert cleared()
    be.reconstruct_view_add_from(store, 0, n)
    assert same(got(be), want)
    # a second view_begin starts over
    be.reconstruct_view_begin(views[:2], Wv, Hv)
    assert got(be)[0].shape == (2, Hv, Wv) and cleared()
    be.reconstruct_view_add_from(store, 0, n)
    assert got(be)[0].tobytes() == want[0][:2].tobytes()
    # recon_begin drops the set
    begin(be, case)
    assert status_of(hip, be.reconstruct_view_add, x, y, t) == _lib.ERR_STATE
    be.reconstruct_view_begin(views, Wv, Hv)
    be.reconstruct_view_end()
    assert status_of(hip, be.reconstruct_view_add_from, store, 0, n) == _lib.ERR_STATE
    be.reconstruct_end()
    store.close()


# ---------------------------------------------------------------- 8. status codes
def test_status_codes(hip, oracle):
    name = "frames8"
    case, Wv, Hv, views = vc.view_set(oracle, name)
    c, (w, x, y, t) = rc.CASES[case], rc.window(case)
    n = c["N"]
    L = _lib.lib()
    be, store = make(hip, case, True), store_of(hip, case)
    # before recon_begin, and on a group handle
    for fn, args in ((be.reconstruct_view_begin, (views, Wv, Hv)), (be.reconstruct_view_add, (x, y, t)), (be.reconstruct_view_get, ()),
                     (be.reconstruct_view_render, (0,)), (be.reconstruct_view_reset, ()), (be.reconstruct_view_end, ())):
        assert status_of(hip, fn, *args) == _lib.ERR_STATE, fn.__name__
    grp = hip.BackendEvaluator(W, H, w.lut, c["Wp"], c["Hp"], devices=[0, 0], transport=_lib.GROUP_DIRECT)
    assert status_of(hip, grp.reconstruct_view_begin, views, Wv, Hv) == _lib.ERR_STATE
    assert status_of(hip, grp.reconstruct_view_add, x, y, t) == _lib.ERR_STATE
    assert status_of(hip, grp.reconstruct_view_get) == _lib.ERR_STATE
    grp.close()
    begin(be, case)
    # before view_begin
    for fn, args in ((be.reconstruct_view_add, (x, y, t)), (be.reconstruct_view_add_aos, (_lib.dvs_events(x, y, t),)),
                     (be.reconstruct_view_add_from, (store, 0, n)), (be.reconstruct_view_get, ()), (be.reconstruct_view_render, (0,)),
                     (be.reconstruct_view_reset, ())):
        assert status_of(hip, fn, *args) == _lib.ERR_STATE, fn.__name__
    # every argument rule of begin
    q, fx, fy, cx, cy, lo, hi = views[0]
    nan, inf = float("nan"), float("inf")
    bad_sets = [([views[0]], 3, 64), ([views[0]], 64, 3), ([views[0]], 8193, 64), ([views[0]], 64, 8193), ([], 64, 64),
                ([views[0]] * 4097, 4, 4), ([views[0]] * 5, 8192, 8192),  # 5 * 2^26 cells > 2^28
                ([(np.zeros(4), fx, fy, cx, cy, lo, hi)], Wv, Hv), ([(np.array([0, nan, 0, 1.0]), fx, fy, cx, cy, lo, hi)], Wv, Hv),
                ([(np.array([0, inf, 0, 1.0]), fx, fy, cx, cy, lo, hi)], Wv, Hv),
                ([(q, 0.0, fy, cx, cy, lo, hi)], Wv, Hv), ([(q, fx, -1.0, cx, cy, lo, hi)], Wv, Hv), ([(q, nan, fy, cx, cy, lo, hi)], Wv, Hv),
                ([(q, fx, inf, cx, cy, lo, hi)], Wv, Hv), ([(q, fx, fy, nan, cy, lo, hi)], Wv, Hv), ([(q, fx, fy, cx, inf, lo, hi)], Wv, Hv),
                ([(q, fx, fy, cx, cy, hi, hi)], Wv, Hv), ([(q, fx, fy, cx, cy, hi, lo)], Wv, Hv),
                ([views[0], (q, fx, fy, cx, cy, hi, lo)], Wv, Hv)]
    for vs, wv, hv in bad_sets:
        assert status_of(hip, be.reconstruct_view_begin, vs, wv, hv) == _lib.ERR_INVALID_ARG, (len(vs), wv, hv)
    assert status_of(hip, be.reconstruct_view_get) == _lib.ERR_STATE  # a refused begin makes no set
    assert L.cmx_backend_recon_view_begin(be._ctx, Wv, Hv, 1, None) == _lib.ERR_INVALID_ARG
    be.reconstruct_view_begin([((0, 0, 0, 2.0), fx, fy, cx, cy, lo, hi)], 4, 8192)  # the limits themselves; any length of quaternion
    be.reconstruct_view_begin(views, Wv, Hv)
    be.reconstruct_view_add_from(store, 0, n)
    snap = got(be)
    assert (snap[1] > 0).all()

    def untouched():
        assert same(got(be), snap)

    try:
        assert L.cmx_diag_set(_lib.DIAG_RECON_SLICE_EVENTS, 4096) == 0   # several slices: the bad event sits in the last one
        bad_x = x.copy()
        bad_x[-2] = W
        assert status_of(hip, be.reconstruct_view_add, bad_x, y, t) == _lib.ERR_EVENT_RANGE
        bad_y = y.copy()
        bad_y[-2] = H
        assert status_of(hip, be.reconstruct_view_add_aos, _lib.dvs_events(x, bad_y, t)) == _lib.ERR_EVENT_RANGE
        untouched()
        back = t.copy()
        back[n - 107] = t[n - 8] + 1000  # the first event of the last batch later than its last one
        assert (n - 107) % c["batch"] == 0
        assert status_of(hip, be.reconstruct_view_add, x, y, back) == _lib.ERR_TIME_ORDER
        st = hip.EventStore(W, H, n)
        st.push(x, y, back)
        assert status_of(hip, be.reconstruct_view_add_from, st, 0, n) == _lib.ERR_TIME_ORDER
        st.close()
        untouched()
        tail = t.copy()
        tail[-150:] += 10_000_000_000  # batch times outside the spline: the last two batches alone
        assert status_of(hip, be.reconstruct_view_add, x, y, tail) == _lib.ERR_SPLINE_RANGE
        assert status_of(hip, be.reconstruct_view_add_aos, _lib.dvs_events(x, y, tail)) == _lib.ERR_SPLINE_RANGE
        st = hip.EventStore(W, H, n)
        st.push(x, y, tail)
        assert status_of(hip, be.reconstruct_view_add_from, st, 0, n) == _lib.ERR_SPLINE_RANGE
        st.close()
        untouched()
    finally:
        assert L.cmx_diag_set(_lib.DIAG_RECON_SLICE_EVENTS, 0) == 0
    assert status_of(hip, be.reconstruct_view_add_from, store, 0, n + 1) == _lib.ERR_INVALID_ARG
    # get and render arguments
    for first, count in ((-1, 1), (0, 9), (8, 1), (9, 0), (0, -1)):
        assert status_of(hip, be.reconstruct_view_get, first, count) == _lib.ERR_INVALID_ARG, (first, count)
    assert be.reconstruct_view_get(8, 0).shape == (0, Hv, Wv)
    for view, gamma in ((-1, 0.75), (8, 0.75), (0, 0.0), (0, -1.0), (0, nan), (0, inf)):
        assert status_of(hip, be.reconstruct_view_render, view, gamma) == _lib.ERR_INVALID_ARG, (view, gamma)
    assert L.cmx_backend_recon_view_render(be._ctx, 0, 0.75, None) == _lib.ERR_INVALID_ARG
    counts_only = np.zeros(8, np.int64)
    assert L.cmx_backend_recon_view_get(be._ctx, 0, 8, None, counts_only.ctypes.data_as(_lib.c_i64p)) == _lib.OK
    assert np.array_equal(counts_only, snap[1])
    untouched()
    be.reconstruct_end()
    store.close()


# ---------------------------------------------------------------- 9. render
@pytest.mark.parametrize("name", ["frames8", "full"])
def test_render_is_the_tone_map_of_the_plane(hip, oracle, name):
    case, Wv, Hv, views = vc.view_set(oracle, name)
    c = rc.CASES[case]
    be, store = make(hip, case, True), store_of(hip, case)
    begin(be, case)
    be.reconstruct_view_begin(views, Wv, Hv)
    assert (be.reconstruct_view_render(0) == 255).all()  # nothing voted: no range
    be.reconstruct_view_add_from(store, 0, c["N"])
    planes = be.reconstruct_view_get()
    other = hip.BackendEvaluator(W, H, rc.window(case)[0].lut, Wv, Hv)  # the map's own render on the same plane
    for k in (0, len(views) - 1):
        other.setIG(planes[k])
        for gamma in (1.0, 0.75):
            img = be.reconstruct_view_render(k, gamma)
            assert img.shape == (Hv, Wv) and img.dtype == np.uint8 and img.min() == 0 and img.max() == 255
            display_ref.assert_levels(img, display_ref.pano_levels(planes[k], gamma), inverted=True,
                                      verbose="%s view %d gamma %.2f" % (name, k, gamma))
            np.testing.assert_array_equal(img, other.publishEventImage(gamma))
    assert be.reconstruct_view_get().tobytes() == planes.tobytes()  # render leaves the planes alone
    be.reconstruct_end()
    store.close()


# ---------------------------------------------------------------- helpers of the public interface
def test_frame_and_crop_helpers(hip, oracle):
    case = "A"
    c, (w, x, y, t) = rc.CASES[case], rc.window(case)
    period = 500_000_000
    views = trajectory.frame_views(c["order"], w.knots_true, w.start_ns, w.dt_ns, period, (200.0, 200.0, 119.75, 89.75))
    support = (c["K"] - c["order"] + 1) * w.dt_ns
    assert len(views) == -(-support // period)
    assert views[0].t_lo_ns == w.start_ns and views[-1].t_hi_ns == w.start_ns + support
    assert all(a.t_hi_ns == b.t_lo_ns for a, b in zip(views[:-1], views[1:]))
    mid = views[3].t_lo_ns + (views[3].t_hi_ns - views[3].t_lo_ns) // 2
    assert np.allclose(np.array(views[3].quat_xyzw), vc.spline_pose(oracle, case, mid), atol=1e-12)
    wide = trajectory.frame_views(c["order"], w.knots_true, w.start_ns, w.dt_ns, period, (200.0, 200.0, 119.75, 89.75),
                                  exposure_ns=2 * period)
    assert [v.t_hi_ns - v.t_lo_ns for v in wide[:-1]] == [2 * period] * (len(wide) - 1) and wide[1].t_lo_ns < views[1].t_lo_ns
    crop = trajectory.crop_view(w.knots_true[50], 20.0, 128, 96)
    assert abs(crop.fx - 64 / np.tan(np.radians(10.0))) < 1e-9 and crop.fx == crop.fy and (crop.cx, crop.cy) == (63.5, 47.5)
    # the helper's structures vote what the same views as tuples vote
    as_tuples = [(np.array(v.quat_xyzw), v.fx, v.fy, v.cx, v.cy, v.t_lo_ns, v.t_hi_ns) for v in views + [crop]]
    _, ref_counts, _, _ = vc.reference_of(oracle, case, as_tuples[:-1], W, H, x, y, t)
    be = make(hip, case, True)
    begin(be, case)
    be.reconstruct_view_begin(views, W, H)
    be.reconstruct_view_add(x, y, t)
    assert np.array_equal(got(be)[1], ref_counts) and (ref_counts > 1000).all()
    be.reconstruct_view_begin([crop], 128, 96)
    be.reconstruct_view_add(x, y, t)
    _, ref_crop, _, _ = vc.reference_of(oracle, case, as_tuples[-1:], 128, 96, x, y, t)
    assert np.array_equal(got(be)[1], ref_crop) and ref_crop[0] >= 100
    be.reconstruct_end()


# ---------------------------------------------------------------- 10. example
def test_example_writes_frames_and_a_crop(hip, tmp_path):
    ex = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples")
    if ex not in sys.path:
        sys.path.insert(0, ex)
    import rotation_pipeline as rp
    stream = synth.event_stream(2e6, 0.5, 240, 180, 200.0, 200.0, 119.5, 89.5, omega_mean=(0.2, 1.8, 0.3), omega_amp=(1.0, 0.8, 1.0), seed=77)
    frames, crop = str(tmp_path / "frame"), str(tmp_path / "crop")
    res = rp.run_pipeline(stream, rp.Params(), frames=frames, frame_ms=50.0, crop=crop)
    planes, counts = res["frames"]
    assert planes.shape[1:] == (180, 240) and len(counts) >= 5
    print("example: %d frames, %s events each; crop %d events" % (len(counts), counts.tolist(), res["crop"][1]))
    assert (counts > 0).all()  # no frame inside the recording is empty
    head = b"P5\n240 180\n255\n"
    for k in range(len(counts)):
        pgm = open("%s_%04d.pgm" % (frames, k), "rb").read()
        assert pgm.startswith(head) and len(pgm) == len(head) + 240 * 180
        img = np.frombuffer(pgm[len(head):], np.uint8)
        assert img.min() == 0 and img.max() == 255
    assert not os.path.exists("%s_%04d.pgm" % (frames, len(counts)))
    cw, ch = rp.CROP_SIZE
    pgm = open(crop + ".pgm", "rb").read()
    head = b"P5\n%d %d\n255\n" % (cw, ch)
    assert pgm.startswith(head) and len(pgm) == len(head) + cw * ch
    assert res["crop"][0].shape == (ch, cw) and res["crop"][1] > 0 and np.frombuffer(pgm[len(head):], np.uint8).min() == 0
    text = open(os.path.join(ex, "rotation_pipeline.py")).read()
    assert "--frames" in text and "--frame-ms" in text and "--crop" in text
