"""GPU: the signed polarity panorama (cmx_backend_recon_pol_* / BackendEvaluator.reconstruct_pol_*, EventStore.push(polarity=)):
the vote loop of reconstruct_add into an ON and an OFF plane.

The main check needs no tolerance: in deterministic mode a plane is a sum of integers, so the coordinates of the per-event export
(reconstruct_warp, itself held against the vote kernel bit for bit by tests/test_gpu_recon_warp.py) with flags == 3, split by
polarity and put through the vote arithmetic on the host (to_fix of cmx_fixed.hpp, an int64 sum per cell), must give the ON and the
OFF plane BIT FOR BIT and both counters exactly.  Beside it: polarity all ones / all zeros against reconstruct_add, the numpy
reference of tests/recon_pol_cases.py in default mode, every ingest path, internal slices, the edge counts, that the calls change
nothing else, that a store with polarity serves every existing consumer as before, the error codes, the tone map, the example.

Bounds.  Default mode: RTOL of tests/util.py on rel_img, the bound every fp32-atomic plane of this suite is held to against its
numpy reference (summation order only; the cell and weights are the export's).  Render on a voted plane: one grey level -- the
restatement and the kernel both evaluate (|s| / m)^gamma in fp32 with pow functions that may differ in the last bit, which can move a
value across a rounding boundary by one level and no further.  Everything else is bitwise."""
import os
import sys

import numpy as np
import pytest

import recon_cases as rc
import recon_pol_cases as pc
import recon_warp_cases as wc
from cmax_slam_amd import _lib, synth
from util import RTOL, rel_img

pytestmark = pytest.mark.gpu
W, H = rc.SENSOR[:2]


def make(hip, name, deterministic=False):
    c, w = rc.CASES[name], rc.window(name)[0]
    be = hip.BackendEvaluator(W, H, w.lut, c["Wp"], c["Hp"])
    if deterministic:
        be.set_deterministic(True)
    return be


def begin(be, name, knots=None):
    c, w = rc.CASES[name], rc.window(name)[0]
    be.reconstruct_begin(c["order"], w.knots_true if knots is None else knots, w.start_ns, w.dt_ns, c["batch"], c["rate"])


def store_of(hip, name, pol="case", capacity=None):
    """the configuration's stream in an EventStore: with its polarity, with the given one, or (pol=None) without any"""
    _, x, y, t = rc.window(name)
    store = hip.EventStore(W, H, capacity or max(len(x), 1))
    if len(x):
        store.push(x, y, t, polarity=pc.polarity(name) if isinstance(pol, str) else pol)
    return store


def status_of(hip, fn, *a, **k):
    with pytest.raises(hip.CmaxHipError) as e:
        fn(*a, **k)
    return e.value.status


def same(a, b):
    """two results of reconstruct_pol_get(with_counts=True), bit for bit"""
    return a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and tuple(a[2:]) == tuple(b[2:])


def voted(hip, name, deterministic=True):
    """reconstruct_pol_get(with_counts=True) after one pol_add_from over the configuration's whole stream"""
    be, store = make(hip, name, deterministic), store_of(hip, name)
    begin(be, name)
    be.reconstruct_pol_add_from(store, 0, rc.CASES[name]["N"])
    out = be.reconstruct_pol_get(with_counts=True)
    be.reconstruct_end()
    store.close()
    return out


def host_fixed_plane(xy, m, Hp, Wp):
    """the deterministic plane of the events selected by m from exported coordinates: vote4_global_fix + recon_fixed_to_float"""
    px, py = xy[m, 0], xy[m, 1]
    xx, yy = px.astype(np.int64), py.astype(np.int64)          # (int)p: truncation, p > 0 here
    dx, dy = (px - xx).astype(np.float32), (py - yy).astype(np.float32)
    one, scale, half = np.float32(1), np.float32(2.0 ** 30), np.float32(0.5)
    w = np.stack([(one - dx) * (one - dy), dx * (one - dy), (one - dx) * dy, dx * dy], axis=1)
    fix = (w * scale + half).astype(np.float32).astype(np.uint32).astype(np.int64)   # to_fix
    acc = np.zeros(Hp * Wp, np.int64)
    for k, (oy, ox) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
        np.add.at(acc, (yy + oy) * Wp + (xx + ox), fix[:, k])
    return (acc.astype(np.float64) * 2.0 ** -30).astype(np.float32).reshape(Hp, Wp)


def bits_differ(a, b):
    return int(np.count_nonzero(a.view(np.uint32) != b.view(np.uint32)))


# ---------------------------------------------------------------- 1. bitwise closure
@pytest.mark.parametrize("name", wc.CLOSURE)
def test_exported_coordinates_split_by_polarity_rebuild_both_planes(hip, name):
    c, pol = rc.CASES[name], pc.polarity(name)
    be, store = make(hip, name, deterministic=True), store_of(hip, name)
    begin(be, name)
    be.reconstruct_pol_add_from(store, 0, c["N"])
    on, off, n_on, n_off = be.reconstruct_pol_get(with_counts=True)
    xy, fl = be.reconstruct_warp_from(store, 0, c["N"])
    be.reconstruct_end()
    store.close()
    m_on, m_off = (fl == 3) & (pol != 0), (fl == 3) & (pol == 0)
    d_on = bits_differ(host_fixed_plane(xy, m_on, c["Hp"], c["Wp"]), on)
    d_off = bits_differ(host_fixed_plane(xy, m_off, c["Hp"], c["Wp"]), off)
    print("%s: %d ON / %d OFF events voted; %d / %d plane cells differ in bits" % (name, n_on, n_off, d_on, d_off))
    assert (n_on, n_off) == (int(np.count_nonzero(m_on)), int(np.count_nonzero(m_off))) and n_on > 0 and n_off > 0
    assert d_on == 0 and d_off == 0


# ---------------------------------------------------------------- 2. one polarity only: the count plane
@pytest.mark.parametrize("name", ["A", "B", "batch5000", "n65"])
def test_a_single_polarity_is_the_count_plane(hip, name):
    c = rc.CASES[name]
    _, x, y, t = rc.window(name)
    be = make(hip, name, deterministic=True)
    begin(be, name)
    be.reconstruct_add(x, y, t)
    plane, _, n_inside = be.reconstruct_get(with_counts=True)
    assert n_inside > 0
    for value in (1, 0):
        be.reconstruct_pol_reset()
        be.reconstruct_pol_add(x, y, t, np.full(c["N"], value, np.uint8))
        on, off, n_on, n_off = be.reconstruct_pol_get(with_counts=True)
        full, empty = (on, off) if value else (off, on)
        assert full.tobytes() == plane.tobytes() and not empty.any()
        assert (n_on, n_off) == ((n_inside, 0) if value else (0, n_inside))
    be.reconstruct_end()


# ---------------------------------------------------------------- 3. default mode against the numpy reference
@pytest.mark.parametrize("name", pc.DEFAULT_MODE)
def test_default_mode_against_the_numpy_reference(hip, oracle, name):
    c = rc.CASES[name]
    _, x, y, t = rc.window(name)
    ref_on, ref_off, ref_n_on, ref_n_off = pc.reference(oracle, name)
    be = make(hip, name)
    begin(be, name)
    be.reconstruct_add(x, y, t)
    n_inside = be.reconstruct_get(with_counts=True)[2]
    be.reconstruct_pol_add(x, y, t, pc.polarity(name))
    on, off, n_on, n_off = be.reconstruct_pol_get(with_counts=True)
    be.reconstruct_end()
    r_on, r_off = rel_img(on, ref_on), rel_img(off, ref_off)
    print("%s: ON %.2e, OFF %.2e against the reference; %d + %d voted, recon_add %d" % (name, r_on, r_off, n_on, n_off, n_inside))
    assert r_on < RTOL and r_off < RTOL
    assert n_on + n_off == n_inside
    assert abs(n_on - ref_n_on) <= wc.MAX_NEAR_INTEGER and abs(n_off - ref_n_off) <= wc.MAX_NEAR_INTEGER


# ---------------------------------------------------------------- 4. ingest paths
@pytest.mark.parametrize("name", ["A", "B", "n65"])
def test_ingest_paths_give_the_same_bytes(hip, name):
    c, pol = rc.CASES[name], pc.polarity(name)
    _, x, y, t = rc.window(name)
    n = c["N"]
    want = voted(hip, name)  # a store filled by push(polarity=)
    assert want[2] > 0 and want[3] > 0
    be = make(hip, name, deterministic=True)
    begin(be, name)

    def fresh(fn, *a, **k):
        be.reconstruct_pol_reset()
        fn(*a, **k)
        return be.reconstruct_pol_get(with_counts=True)

    assert same(fresh(be.reconstruct_pol_add, x, y, t, pol), want)
    assert same(fresh(be.reconstruct_pol_add, x, y, t, pol * np.uint8(255)), want)  # any nonzero byte is ON
    records = _lib.dvs_events(x, y, t, polarity=pol)
    assert same(fresh(be.reconstruct_pol_add_aos, records), want)
    # a store filled from the records
    st = hip.EventStore(W, H, n)
    assert not st.has_polarity
    st.push_aos(records, polarity_field="polarity")
    assert st.has_polarity
    assert same(fresh(be.reconstruct_pol_add_from, st, 0, n), want)
    st.close()
    # a range that starts behind a drop_before compaction: a prefix with the OPPOSITE polarity is pushed, then dropped
    k = 777 if n > 777 else 7
    st = hip.EventStore(W, H, n + k)
    st.push(x[:k], y[:k], t[:k], polarity=1 - pol[:k])
    st.push(x[:n // 2], y[:n // 2], t[:n // 2], polarity=pol[:n // 2])
    st.drop_before(k)
    st.push(x[n // 2:], y[n // 2:], t[n // 2:], polarity=pol[n // 2:])
    assert (st.begin, st.end) == (k, k + n) and st.has_polarity
    assert same(fresh(be.reconstruct_pol_add_from, st, k, n), want)
    # ... and a sub-range off the batch grid against the same events from host arrays
    lo, m = 7 * 64 + 1, 5 * 64 + 1
    if n >= lo + m:
        sub = fresh(be.reconstruct_pol_add_from, st, k + lo, m)
        assert same(fresh(be.reconstruct_pol_add, x[lo:lo + m], y[lo:lo + m], t[lo:lo + m], pol[lo:lo + m]), sub) and sub[2] + sub[3] > 0
    st.close()
    be.reconstruct_end()


# ---------------------------------------------------------------- 5. slices
@pytest.mark.parametrize("name", ["A", "B"])
def test_internal_slices_and_cuts_change_nothing(hip, name):
    c, pol = rc.CASES[name], pc.polarity(name)
    _, x, y, t = rc.window(name)
    n, B = c["N"], c["batch"]
    want = voted(hip, name)
    be, store = make(hip, name, deterministic=True), store_of(hip, name)
    begin(be, name)
    L = _lib.lib()
    records = _lib.dvs_events(x, y, t, polarity=pol)
    try:
        for n_slice in (2 * B, 4096, 0):   # two batches per slice; a few slices; the default (one slice)
            assert L.cmx_diag_set(_lib.DIAG_RECON_SLICE_EVENTS, n_slice) == 0
            for fn, args in ((be.reconstruct_pol_add_from, (store, 0, n)), (be.reconstruct_pol_add, (x, y, t, pol)),
                             (be.reconstruct_pol_add_aos, (records,))):
                be.reconstruct_pol_reset()
                fn(*args)
                assert same(be.reconstruct_pol_get(with_counts=True), want), (n_slice, fn.__name__)
    finally:
        assert L.cmx_diag_set(_lib.DIAG_RECON_SLICE_EVENTS, 0) == 0
    # the stream cut at a batch multiple into two calls
    cut = 37 * B
    be.reconstruct_pol_reset()
    be.reconstruct_pol_add_from(store, 0, cut)
    be.reconstruct_pol_add_from(store, cut, n - cut)
    assert same(be.reconstruct_pol_get(with_counts=True), want)
    be.reconstruct_pol_reset()
    be.reconstruct_pol_add(x[:cut], y[:cut], t[:cut], pol[:cut])
    be.reconstruct_pol_add_aos(records[cut:])
    assert same(be.reconstruct_pol_get(with_counts=True), want)
    be.reconstruct_end()
    store.close()


# ---------------------------------------------------------------- 6. edge counts
def test_edge_counts(hip, oracle):
    for name in ("n0", "n1", "n2", "n65"):
        c, pol = rc.CASES[name], pc.polarity(name)
        _, x, y, t = rc.window(name)
        n = c["N"]
        be, store = make(hip, name, deterministic=True), store_of(hip, name)
        begin(be, name)
        before = be.reconstruct_pol_get(with_counts=True)   # nothing voted, nothing allocated: zeros
        assert not before[0].any() and not before[1].any() and before[2:] == (0, 0)
        be.reconstruct_add(x, y, t)
        n_inside = be.reconstruct_get(with_counts=True)[2]
        be.reconstruct_pol_add(x, y, t, pol)
        host = be.reconstruct_pol_get(with_counts=True)
        be.reconstruct_pol_reset()
        be.reconstruct_pol_add_aos(_lib.dvs_events(x, y, t, polarity=pol))
        assert same(be.reconstruct_pol_get(with_counts=True), host)
        be.reconstruct_pol_reset()
        be.reconstruct_pol_add_from(store, 0, n)     # (n0: an empty store holds no polarity and no events: nothing to refuse)
        assert same(be.reconstruct_pol_get(with_counts=True), host)
        be.reconstruct_end()
        store.close()
        assert host[2] + host[3] == n_inside
        ref = pc.reference(oracle, name)
        assert host[2:] == ref[2:]
        if n < 2:   # n0; n1: the lone event votes nowhere
            assert n_inside == 0
        assert host[0].any() == (ref[2] > 0) and host[1].any() == (ref[3] > 0)
        if n_inside:
            assert rel_img(host[0] + host[1], ref[0] + ref[1]) < RTOL
        if name == "n65":
            assert host[2] > 0 and host[3] > 0
    # n65: the 65th event is the lone trailing one -- its polarity votes nowhere
    _, x, y, t = rc.window("n65")
    be = make(hip, "n65", deterministic=True)
    begin(be, "n65")
    pol = np.zeros(65, np.uint8)
    pol[64] = 1
    be.reconstruct_pol_add(x, y, t, pol)
    on, off, n_on, n_off = be.reconstruct_pol_get(with_counts=True)
    assert n_on == 0 and not on.any() and n_off > 0
    be.reconstruct_end()


# ---------------------------------------------------------------- 7. the calls change nothing else
def pol_calls(be, store, n):
    be.reconstruct_pol_add_from(store, 0, n)
    out = be.reconstruct_pol_get(with_counts=True)
    be.reconstruct_pol_render(0.75, 0)
    be.reconstruct_pol_render(0.75, 1)
    return out


def test_the_polarity_calls_change_nothing_else(hip):
    name = "window"
    c, (w, x, y, t) = rc.CASES[name], rc.window(name)
    n = c["N"]
    once = voted(hip, name)
    be, store = make(hip, name, deterministic=True), store_of(hip, name)
    zero = np.zeros(3 * c["K"])
    be.set_window(x[:5000], y[:5000], t[:5000], c["order"], w.knots_true, w.start_ns, w.dt_ns, 0, 2 ** 62, c["batch"], c["rate"])
    win_before = be.eval(zero)
    begin(be, name)
    # the count plane and its counters; an open gradient pass with half of its events added
    be.reconstruct_add_from(store, 0, n)
    be.reconstruct_contrast(1.0, want_grad=True)
    be.reconstruct_grad_add_from(store, 0, 10_000)
    state = be.reconstruct_get(with_counts=True)
    assert same(pol_calls(be, store, n), once)
    be.reconstruct_grad_add_from(store, 10_000, n - 10_000)
    grad = be.reconstruct_grad_get()  # (CMX_ERR_STATE had a polarity call closed the pass or touched its counts)
    assert np.abs(grad).max() > 0
    be.reconstruct_pol_reset()
    assert same(pol_calls(be, store, n), once)
    assert be.reconstruct_grad_get().tobytes() == grad.tobytes()
    now = be.reconstruct_get(with_counts=True)
    assert now[0].tobytes() == state[0].tobytes() and now[1:] == state[1:]
    # the same sums from a run without any polarity call in between
    ref = make(hip, name, deterministic=True)
    begin(ref, name)
    ref.reconstruct_add_from(store, 0, n)
    ref.reconstruct_contrast(1.0, want_grad=True)
    ref.reconstruct_grad_add_from(store, 0, 10_000)
    ref.reconstruct_grad_add_from(store, 10_000, n - 10_000)
    assert ref.reconstruct_grad_get().tobytes() == grad.tobytes()
    # bound events, without and with a frozen head, and after release_head: eval_bound is bitwise what it is without the calls
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
        state = be.reconstruct_get(with_counts=True)
        be.reconstruct_pol_reset()
        assert same(pol_calls(be, store, n), once), step
        assert (be.reconstruct_bound_info(), be.reconstruct_frozen_info(), be.reconstruct_online_info()) == infos
        now = be.reconstruct_get(with_counts=True)
        assert now[0].tobytes() == state[0].tobytes() and now[1:] == state[1:]
        ev2, ev_ref = be.reconstruct_eval_bound(None, 1.0), ref.reconstruct_eval_bound(None, 1.0)
        assert ev2[0] == ev[0] == ev_ref[0] and ev2[1].tobytes() == ev[1].tobytes() == ev_ref[1].tobytes(), step
        assert be.reconstruct_bound_info()["sorts"] == infos[0]["sorts"]  # (the tile sort survived)
        assert same(be.reconstruct_pol_get(with_counts=True), once)        # eval_bound leaves the polarity planes alone
        if step == "frozen":
            assert infos[1]["frozen_batches"] > 0
        if step == "released":
            assert infos[2]["released_sampled"] > 0
    ref.reconstruct_end()
    # pol_reset clears the two planes and their counters and nothing else
    state = be.reconstruct_get(with_counts=True)
    be.reconstruct_pol_reset()
    cleared = be.reconstruct_pol_get(with_counts=True)
    assert not cleared[0].any() and not cleared[1].any() and cleared[2:] == (0, 0)
    now = be.reconstruct_get(with_counts=True)
    assert now[0].tobytes() == state[0].tobytes() and now[1:] == state[1:]
    ev3 = be.reconstruct_eval_bound(None, 1.0)
    assert ev3[0] == ev[0] and ev3[1].tobytes() == ev[1].tobytes()
    # the window evaluation is where it was
    win_after = be.eval(zero)
    assert win_after[0] == win_before[0] and win_after[1].tobytes() == win_before[1].tobytes()
    be.reconstruct_end()
    # restart clears the planes (votes under other knots are stale), and what is voted then is the reference at the new knots
    begin(be, name)
    assert same(pol_calls(be, store, n), once)
    be.reconstruct_restart(w.knots_true)
    cleared = be.reconstruct_pol_get(with_counts=True)
    assert not cleared[0].any() and not cleared[1].any() and cleared[2:] == (0, 0)
    assert same(pol_calls(be, store, n), once)
    # a second begin starts over; end frees
    begin(be, name)
    cleared = be.reconstruct_pol_get(with_counts=True)
    assert not cleared[0].any() and cleared[2:] == (0, 0)
    be.reconstruct_end()
    assert status_of(hip, be.reconstruct_pol_get) == _lib.ERR_STATE
    store.close()


# ---------------------------------------------------------------- 8. a store with polarity serves every existing consumer as before
def test_a_store_with_polarity_serves_existing_consumers_identically(hip):
    name = "window"
    c, (w, x, y, t) = rc.CASES[name], rc.window(name)
    n = c["N"]
    zero = np.zeros(3 * (c["K"] - 2))
    results = []
    for pol in (None, "case"):
        be, store = make(hip, name, deterministic=True), store_of(hip, name, pol=pol)
        assert store.has_polarity == (pol is not None)
        be.set_window_from(store, 0, 8000, c["order"], w.knots_true, w.start_ns, w.dt_ns, 2, int(t[4000]), c["batch"], c["rate"])
        win = be.eval(zero)
        begin(be, name)
        be.reconstruct_add_from(store, 0, n)
        plane = be.reconstruct_get(with_counts=True)
        xy, fl = be.reconstruct_warp_from(store, 0, n)
        be.reconstruct_bind(store, 0, n)
        ev = be.reconstruct_eval_bound(None, 1.0)
        be.reconstruct_end()
        store.close()
        results.append((win, plane, xy, fl, ev))
    (win0, plane0, xy0, fl0, ev0), (win1, plane1, xy1, fl1, ev1) = results
    assert win0[0] == win1[0] and win0[1].tobytes() == win1[1].tobytes() and np.abs(win0[1]).max() > 0
    assert plane0[0].tobytes() == plane1[0].tobytes() and plane0[1:] == plane1[1:] and plane0[2] > 0
    assert xy0.tobytes() == xy1.tobytes() and fl0.tobytes() == fl1.tobytes()
    assert ev0[0] == ev1[0] and ev0[1].tobytes() == ev1[1].tobytes() and np.abs(ev0[1]).max() > 0


# ---------------------------------------------------------------- 9. errors add nothing
def test_errors_add_nothing(hip):
    name = "window"
    c, (w, x, y, t) = rc.CASES[name], rc.window(name)
    n, pol = c["N"], pc.polarity(name)
    L = _lib.lib()
    be, store = make(hip, name, deterministic=True), store_of(hip, name)
    plain = store_of(hip, name, pol=None)
    # before begin, and on a group handle
    assert status_of(hip, be.reconstruct_pol_add, x, y, t, pol) == _lib.ERR_STATE
    assert status_of(hip, be.reconstruct_pol_add_from, store, 0, n) == _lib.ERR_STATE
    assert status_of(hip, be.reconstruct_pol_render) == _lib.ERR_STATE
    assert status_of(hip, be.reconstruct_pol_reset) == _lib.ERR_STATE
    grp = hip.BackendEvaluator(W, H, w.lut, c["Wp"], c["Hp"], devices=[0, 0], transport=_lib.GROUP_DIRECT)
    assert status_of(hip, grp.reconstruct_pol_add, x, y, t, pol) == _lib.ERR_STATE
    assert status_of(hip, grp.reconstruct_pol_add_aos, _lib.dvs_events(x, y, t, polarity=pol)) == _lib.ERR_STATE
    assert status_of(hip, grp.reconstruct_pol_get) == _lib.ERR_STATE
    grp.close()
    begin(be, name)
    be.reconstruct_pol_add_from(store, 0, n)
    snap = be.reconstruct_pol_get(with_counts=True)
    assert snap[2] > 0 and snap[3] > 0

    def untouched():
        assert same(be.reconstruct_pol_get(with_counts=True), snap)

    try:
        assert L.cmx_diag_set(_lib.DIAG_RECON_SLICE_EVENTS, 4096) == 0   # five slices: the bad event sits in the last one
        # an event outside the sensor in the last slice (an unsampled position counts too)
        bad_x = x.copy()
        bad_x[-2] = W
        assert status_of(hip, be.reconstruct_pol_add, bad_x, y, t, pol) == _lib.ERR_EVENT_RANGE
        bad_y = y.copy()
        bad_y[-2] = H
        assert status_of(hip, be.reconstruct_pol_add_aos, _lib.dvs_events(x, bad_y, t, polarity=pol)) == _lib.ERR_EVENT_RANGE
        untouched()
        # a batch whose first event is later than its last one, in the last slice
        back = t.copy()
        back[19_900] = t[19_999] + 1000
        assert status_of(hip, be.reconstruct_pol_add, x, y, back, pol) == _lib.ERR_TIME_ORDER
        st = hip.EventStore(W, H, n)
        st.push(x, y, back, polarity=pol)
        assert status_of(hip, be.reconstruct_pol_add_from, st, 0, n) == _lib.ERR_TIME_ORDER
        st.close()
        untouched()
        # batch times outside the spline: the last two batches alone
        tail = t.copy()
        tail[-150:] += 10_000_000_000
        assert status_of(hip, be.reconstruct_pol_add, x, y, tail, pol) == _lib.ERR_SPLINE_RANGE
        assert status_of(hip, be.reconstruct_pol_add_aos, _lib.dvs_events(x, y, tail, polarity=pol)) == _lib.ERR_SPLINE_RANGE
        st = hip.EventStore(W, H, n)
        st.push(x, y, tail, polarity=pol)
        assert status_of(hip, be.reconstruct_pol_add_from, st, 0, n) == _lib.ERR_SPLINE_RANGE
        st.close()
        untouched()
    finally:
        assert L.cmx_diag_set(_lib.DIAG_RECON_SLICE_EVENTS, 0) == 0
    # a store without polarity; ranges and arguments
    assert not plain.has_polarity
    assert status_of(hip, be.reconstruct_pol_add_from, plain, 0, n) == _lib.ERR_STATE
    assert status_of(hip, be.reconstruct_pol_add_from, store, 0, n + 1) == _lib.ERR_INVALID_ARG
    assert L.cmx_backend_recon_pol_add(be._ctx, n, x.ctypes.data_as(_lib.c_u16p), y.ctypes.data_as(_lib.c_u16p),
                                       t.ctypes.data_as(_lib.c_i64p), None) == _lib.ERR_INVALID_ARG
    records = _lib.dvs_events(x, y, t, polarity=pol)
    lay = _lib.aos_layout_of(records)
    assert L.cmx_backend_recon_pol_add_aos(be._ctx, n, records.ctypes.data, lay, 16) == _lib.ERR_INVALID_ARG
    untouched()
    # mixing the two kinds of push: CMX_ERR_STATE, nothing is pushed, and the store serves as before
    assert status_of(hip, store.push, x[:10], y[:10], t[:10]) == _lib.ERR_STATE
    assert status_of(hip, store.push_aos, records[:10]) == _lib.ERR_STATE
    assert status_of(hip, plain.push, x[:10], y[:10], t[:10], pol[:10]) == _lib.ERR_STATE
    assert status_of(hip, plain.push_aos, records[:10], "polarity") == _lib.ERR_STATE
    assert (store.begin, store.end, store.has_polarity) == (0, n, True) and (plain.begin, plain.end, plain.has_polarity) == (0, n, False)
    be.reconstruct_pol_reset()
    be.reconstruct_pol_add_from(store, 0, n)
    untouched()
    # once a store is empty again, the next push decides anew
    plain.drop_before(n)
    plain.push(x[:10], y[:10], t[:10], polarity=pol[:10])
    assert plain.has_polarity and (plain.begin, plain.end) == (n, n + 10)
    # render arguments
    for gamma, mode in ((0.75, 2), (0.75, -1), (0.0, 0), (-1.0, 1), (float("nan"), 0), (float("inf"), 1)):
        assert status_of(hip, be.reconstruct_pol_render, gamma, mode) == _lib.ERR_INVALID_ARG, (gamma, mode)
    assert L.cmx_backend_recon_pol_render(be._ctx, 0.75, 0, None) == _lib.ERR_INVALID_ARG
    untouched()
    be.reconstruct_end()
    store.close()
    plain.close()


# ---------------------------------------------------------------- 10. render
def restate_render(on, off, gamma, mode):
    """the formulas of include/cmax_hip.h in fp32"""
    s = on - off
    assert s.dtype == np.float32
    m = np.float32(np.abs(s).max())
    q = np.abs(s) / m if m > 0 else np.zeros_like(s)
    p = q if gamma == 1.0 else np.power(q, np.float32(gamma))
    assert p.dtype == np.float32
    v = np.copysign(p, s)
    if mode == 0:
        return np.rint(np.float32(127.5) + np.float32(127.5) * v).astype(np.uint8)
    a = np.rint(np.float32(255) * np.abs(v)).astype(np.int64)
    out = np.full(s.shape + (3,), 255, np.int64)
    pos = s > 0
    out[..., 0] = np.where(pos, 255 - a, 255)
    out[..., 1] = 255 - a
    out[..., 2] = np.where(pos, 255, 255 - a)
    return out.astype(np.uint8)


@pytest.mark.parametrize("deterministic", [False, True])
def test_render_of_dyadic_planes_is_exact(hip, deterministic):
    """Hand-made planes reached through real votes: a bearing table whose first three pixels look along +z, +x and -x lands their
    events, under the identity trajectory, on the pixel centres (Wp/2, Hp/2), (3Wp/4, Hp/2), (Wp/4, Hp/2) -- weight 1 on one cell,
    0 on its neighbours -- so the planes hold small integers and s / m is a power of two."""
    Wp, Hp = 256, 128
    lut = np.zeros((H, W, 3))
    lut[..., 2] = 1.0
    lut[0, 1] = (1.0, 0.0, 0.0)
    lut[0, 2] = (-1.0, 0.0, 0.0)
    be = hip.BackendEvaluator(W, H, lut, Wp, Hp)
    if deterministic:
        be.set_deterministic(True)
    knots = np.tile(np.array([0.0, 0.0, 0.0, 1.0]), (4, 1))
    be.reconstruct_begin(4, knots, 0, 1_000_000_000, 3, 1)
    #            cell +z: 4 ON       cell +x: 1 ON, 3 OFF      cell -x: 1 OFF          ->  s = +4, -2, -1;  m = 4
    px = np.array([0, 0, 0, 0,      1, 1, 1, 1,               2], np.uint16)
    pol = np.array([1, 1, 1, 1,     1, 0, 0, 0,               0], np.uint8)
    py = np.zeros(9, np.uint16)
    t = np.arange(9, dtype=np.int64) * 1000 + 1000
    xy, fl = be.reconstruct_warp(px, py, t)
    cells = [(Wp // 2, Hp // 2), (3 * Wp // 4, Hp // 2), (Wp // 4, Hp // 2)]
    assert (fl == 3).all()
    assert np.array_equal(xy, np.array([cells[i] for i in px], np.float64)), xy   # the pixel centres, exactly
    be.reconstruct_pol_add(px, py, t, pol)
    on, off, n_on, n_off = be.reconstruct_pol_get(with_counts=True)
    want_on, want_off = np.zeros((Hp, Wp), np.float32), np.zeros((Hp, Wp), np.float32)
    for (cx, cy), a, b in zip(cells, (4, 1, 0), (0, 3, 1)):
        want_on[cy, cx], want_off[cy, cx] = a, b
    assert on.tobytes() == want_on.tobytes() and off.tobytes() == want_off.tobytes() and (n_on, n_off) == (5, 4)
    for gamma in (1.0, 0.75, 2.0):
        mono, bgr = be.reconstruct_pol_render(gamma, 0), be.reconstruct_pol_render(gamma, 1)
        assert mono.shape == (Hp, Wp) and bgr.shape == (Hp, Wp, 3) and mono.dtype == bgr.dtype == np.uint8
        assert np.array_equal(mono, restate_render(on, off, gamma, 0)), gamma
        assert np.array_equal(bgr, restate_render(on, off, gamma, 1)), gamma
        (ax, ay), (bx, by), (cx, cy) = cells
        assert mono[ay, ax] == 255 and mono[0, 0] == 128 and mono[by, bx] < mono[cy, cx] < 128
        assert tuple(bgr[ay, ax]) == (0, 0, 255) and tuple(bgr[0, 0]) == (255, 255, 255)             # ON at full scale: red
        assert bgr[by, bx, 0] == 255 and bgr[by, bx, 1] == bgr[by, bx, 2] < bgr[cy, cx, 1] < 255   # OFF: blue, the stronger the darker
    assert tuple(be.reconstruct_pol_render(1.0, 1)[cells[1][1], cells[1][0]]) == (255, 127, 127)   # a = rint(127.5) = 128
    # an all-zero pair: the neutral image
    be.reconstruct_pol_reset()
    assert (be.reconstruct_pol_render(0.75, 0) == 128).all() and (be.reconstruct_pol_render(0.75, 1) == 255).all()
    be.reconstruct_end()
    be.reconstruct_begin(4, knots, 0, 1_000_000_000, 3, 1)   # ... and before anything has been voted at all
    assert (be.reconstruct_pol_render(0.75, 0) == 128).all() and (be.reconstruct_pol_render(0.75, 1) == 255).all()
    be.reconstruct_end()


@pytest.mark.parametrize("name", ["A", "pano130x96"])
def test_render_of_a_voted_configuration_is_within_one_level(hip, name):
    c = rc.CASES[name]
    be, store = make(hip, name, deterministic=True), store_of(hip, name)
    begin(be, name)
    be.reconstruct_pol_add_from(store, 0, c["N"])
    on, off = be.reconstruct_pol_get()
    for gamma in (0.75, 1.0):
        for mode in (0, 1):
            img = be.reconstruct_pol_render(gamma, mode)
            d = np.abs(img.astype(np.int64) - restate_render(on, off, gamma, mode).astype(np.int64))
            print("%s gamma %.2f mode %d: %d of %d values differ, by at most %d" % (name, gamma, mode, np.count_nonzero(d), d.size, d.max()))
            assert d.max() <= 1
            assert np.count_nonzero(d) <= d.size // 100   # ... and for nearly all of them not at all
    mono = be.reconstruct_pol_render(0.75, 0)
    s = on - off
    assert mono.min() < 64 and mono.max() > 192 and (mono[s == 0] == 128).all() and (mono[s > 0] >= 128).all() and (mono[s < 0] <= 128).all()
    be.reconstruct_end()
    store.close()


# ---------------------------------------------------------------- 11. example
def test_example_writes_the_polarity_map(hip, tmp_path):
    ex = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples")
    if ex not in sys.path:
        sys.path.insert(0, ex)
    import rotation_pipeline as rp
    stream = synth.event_stream(2e6, 0.5, 240, 180, 200.0, 200.0, 119.5, 89.5, omega_mean=(0.2, 1.8, 0.3), omega_amp=(1.0, 0.8, 1.0), seed=77)
    path = str(tmp_path / "polmap")
    res = rp.run_pipeline(stream, rp.Params(), reconstruct=True, polarity_map=path)
    Hp, Wp = res["recon"].shape
    on, off = res["pol"]
    assert on.shape == off.shape == (Hp, Wp) and on.any() and off.any()
    r = rel_img(on.astype(np.float64) + off.astype(np.float64), res["recon"])
    print("example: ON + OFF vs the example's count panorama %.2e" % r)
    assert r < RTOL
    pgm, ppm = open(path + ".pgm", "rb").read(), open(path + ".ppm", "rb").read()
    head = b"P5\n%d %d\n255\n" % (Wp, Hp)
    assert pgm.startswith(head) and len(pgm) == len(head) + Hp * Wp
    head = b"P6\n%d %d\n255\n" % (Wp, Hp)
    assert ppm.startswith(head) and len(ppm) == len(head) + 3 * Hp * Wp
    mono = np.frombuffer(pgm[-Hp * Wp:], np.uint8).reshape(Hp, Wp)
    rgb = np.frombuffer(ppm[-3 * Hp * Wp:], np.uint8).reshape(Hp, Wp, 3)
    s = on - off
    assert (mono[s > 0] >= 128).all() and (mono[s < 0] <= 128).all() and (mono.max() == 255 or mono.min() == 0)
    assert (rgb[s > 0][:, 0] == 255).all() and (rgb[s < 0][:, 2] == 255).all()   # RGB: ON red, OFF blue
    text = open(os.path.join(ex, "rotation_pipeline.py")).read()
    assert "--polarity-map" in text and "seeded" in text
