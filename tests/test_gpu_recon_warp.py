"""GPU: the per-event export (cmx_backend_recon_warp* / BackendEvaluator.reconstruct_warp*): where every event lands under the
knots the reconstruction holds.

The main check needs no tolerance: in deterministic mode the plane of recon_add is a sum of integers, so the exported coordinates of
the events with flags == 3, put through the vote arithmetic on the host (cell = int(p), weight offsets float32(p - cell), four fp32
weights, to_fix of cmx_fixed.hpp, an int64 sum per cell), must give the plane BIT FOR BIT -- any coordinate that is not the vote
kernel's own, any wrong flag, any event out of order shows.  Beside it: the numpy reference of tests/recon_warp_cases.py (checked on
the CPU by tests/test_recon_warp_cpu.py), the two formats, the four ingest paths, internal slices, the edge counts, that the calls
change nothing, the error codes, and the example's --export-warped.

Parity bound (test 2).  Measured on MI355X over all configurations, max |p - p_ref| in pixels over all events
(profiles/recon_warp_parity.txt): 1.4e-14 .. 5.7e-14 for eleven of them, 2.842e-13 for `poles` (votes next to the poles, where asin
is steep) -- the 1e-12 Wp/512 px expected from cmx_trig.hpp's 1-3 ulp.  Asserted: 16 x the largest = 4.55e-12 px (the trig
polynomials' error varies with the octant and the configurations sample few octants), under the cap of 1e-9 px -- 1/30 of half an
fp32 weight ulp, so an export inside it cannot move a vote weight by more than its last bit."""
import os
import sys

import numpy as np
import pytest

import recon_cases as rc
import recon_warp_cases as wc
from cmax_slam_amd import _lib, synth
from util import RTOL, rel_img

pytestmark = pytest.mark.gpu
W, H = rc.SENSOR[:2]

PARITY_MEASURED_MAX = 2.842e-13  # px: the largest of profiles/recon_warp_parity.txt (poles, py)
PARITY_BOUND = min(16 * PARITY_MEASURED_MAX, 1e-9)


def make(hip, name, deterministic=False):
    c, w = rc.CASES[name], rc.window(name)[0]
    be = hip.BackendEvaluator(W, H, w.lut, c["Wp"], c["Hp"])
    if deterministic:
        be.set_deterministic(True)
    return be


def begin(be, name, knots=None):
    c, w = rc.CASES[name], rc.window(name)[0]
    be.reconstruct_begin(c["order"], w.knots_true if knots is None else knots, w.start_ns, w.dt_ns, c["batch"], c["rate"])


def store_of(hip, name):
    _, x, y, t = rc.window(name)
    store = hip.EventStore(W, H, max(len(x), 1))
    if len(x):
        store.push(x, y, t)
    return store


_exports = {}


def export(hip, name):
    """(xy float64 [n, 2], flags) of warp_from over the configuration's whole stream at its true knots (computed once, read-only)"""
    if name not in _exports:
        be, store = make(hip, name), store_of(hip, name)
        begin(be, name)
        out = be.reconstruct_warp_from(store, 0, rc.CASES[name]["N"])
        be.reconstruct_end()
        store.close()
        for a in out:
            a.setflags(write=False)
        _exports[name] = out
    return _exports[name]


def status_of(hip, fn, *a, **k):
    with pytest.raises(hip.CmaxHipError) as e:
        fn(*a, **k)
    return e.value.status


def same_bytes(a, b):
    return a[0].dtype == b[0].dtype and a[0].shape == b[0].shape and a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


def host_fixed_plane(xy, fl, Hp, Wp):
    """the deterministic plane from exported coordinates: vote4_global_fix + recon_fixed_to_float on the host"""
    m = fl == 3
    px, py = xy[m, 0], xy[m, 1]
    xx, yy = px.astype(np.int64), py.astype(np.int64)          # (int)p: truncation, p > 0 here
    dx, dy = (px - xx).astype(np.float32), (py - yy).astype(np.float32)
    one, scale, half = np.float32(1), np.float32(2.0 ** 30), np.float32(0.5)
    w = np.stack([(one - dx) * (one - dy), dx * (one - dy), (one - dx) * dy, dx * dy], axis=1)
    assert w.dtype == np.float32
    fix = (w * scale + half).astype(np.float32).astype(np.uint32).astype(np.int64)   # to_fix
    acc = np.zeros(Hp * Wp, np.int64)
    for k, (oy, ox) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
        np.add.at(acc, (yy + oy) * Wp + (xx + ox), fix[:, k])
    return (acc.astype(np.float64) * 2.0 ** -30).astype(np.float32).reshape(Hp, Wp)


# ---------------------------------------------------------------- 1. bitwise closure
@pytest.mark.parametrize("name", wc.CLOSURE)
def test_exported_coordinates_rebuild_the_plane_bit_for_bit(hip, name):
    c = rc.CASES[name]
    be, store = make(hip, name, deterministic=True), store_of(hip, name)
    begin(be, name)
    be.reconstruct_add_from(store, 0, c["N"])
    plane, n_sampled, n_inside = be.reconstruct_get(with_counts=True)
    xy, fl = be.reconstruct_warp_from(store, 0, c["N"])
    after = be.reconstruct_get(with_counts=True)
    be.reconstruct_end()
    store.close()
    assert xy.shape == (c["N"], 2) and xy.dtype == np.float64 and fl.shape == (c["N"],) and fl.dtype == np.uint8
    assert int(np.count_nonzero(fl & 1)) == n_sampled == rc.sampled(c["N"], c["batch"], c["rate"])
    assert int(np.count_nonzero(fl == 3)) == n_inside > 0
    assert not (fl & ~np.uint8(3)).any()
    host = host_fixed_plane(xy, fl, c["Hp"], c["Wp"])
    diff = int(np.count_nonzero(host.view(np.uint32) != plane.view(np.uint32)))
    print("%s: %d events, %d voted, %d plane cells differ in bits" % (name, c["N"], n_inside, diff))
    assert diff == 0
    assert after[0].tobytes() == plane.tobytes() and after[1:] == (n_sampled, n_inside)


@pytest.mark.parametrize("name", wc.CLOSURE)
def test_exported_coordinates_rebuild_the_default_plane(hip, name):
    """default mode: fp32 atomics, equal up to summation order"""
    c = rc.CASES[name]
    be, store = make(hip, name), store_of(hip, name)
    begin(be, name)
    be.reconstruct_add_from(store, 0, c["N"])
    plane, n_sampled, n_inside = be.reconstruct_get(with_counts=True)
    xy, fl = be.reconstruct_warp_from(store, 0, c["N"])
    be.reconstruct_end()
    store.close()
    assert same_bytes((xy, fl), export(hip, name))  # the export does not depend on the mode
    assert int(np.count_nonzero(fl & 1)) == n_sampled and int(np.count_nonzero(fl == 3)) == n_inside
    r = rel_img(wc.revote(xy[:, 0], xy[:, 1], fl, c["Hp"], c["Wp"]), plane)
    print("%s: host re-vote vs fp32 plane %.2e" % (name, r))
    assert r < RTOL


# ---------------------------------------------------------------- 2. against the numpy reference
@pytest.mark.parametrize("name", wc.ALL)
def test_against_the_numpy_reference(hip, oracle, name):
    c = rc.CASES[name]
    px, py, fl_ref = wc.reference(oracle, name)
    xy, fl = export(hip, name)
    assert xy.shape == (c["N"], 2)
    if c["N"] == 0:
        return
    ex, ey = float(np.abs(xy[:, 0] - px).max()), float(np.abs(xy[:, 1] - py).max())
    print("parity %-11s N %6d  Wp %4d  max|px - ref| %.3e  max|py - ref| %.3e  (all events, unsampled and lone included)" %
          (name, c["N"], c["Wp"], ex, ey))
    assert max(ex, ey) <= PARITY_BOUND
    keep = ~wc.near_integer(px, py)
    assert np.count_nonzero(~keep) <= wc.MAX_NEAR_INTEGER
    np.testing.assert_array_equal(fl[keep], fl_ref[keep])
    np.testing.assert_array_equal(np.trunc(xy[keep]).astype(np.int64), np.stack([np.trunc(px), np.trunc(py)], axis=1).astype(np.int64)[keep])


# ---------------------------------------------------------------- 3. format
@pytest.mark.parametrize("name", ["A", "B", "n65", "batch1"])
def test_f32_is_the_rounded_f64(hip, name):
    c = rc.CASES[name]
    be, store = make(hip, name), store_of(hip, name)
    _, x, y, t = rc.window(name)
    begin(be, name)
    xy32, fl32 = be.reconstruct_warp_from(store, 0, c["N"], dtype=np.float32)
    host32 = be.reconstruct_warp(x, y, t, dtype=np.float32)
    be.reconstruct_end()
    store.close()
    xy, fl = export(hip, name)
    assert xy32.dtype == np.float32 and xy32.shape == (c["N"], 2)
    assert xy32.tobytes() == xy.astype(np.float32).tobytes()
    assert fl32.tobytes() == fl.tobytes()
    assert same_bytes(host32, (xy32, fl32))
    with pytest.raises(ValueError):
        be.reconstruct_warp(x, y, t, dtype=np.float16)


# ---------------------------------------------------------------- 4. ingest paths
@pytest.mark.parametrize("name", ["A", "B", "n65"])
def test_ingest_paths_give_the_same_bytes(hip, name):
    import torch
    c = rc.CASES[name]
    _, x, y, t = rc.window(name)
    n = c["N"]
    be, store = make(hip, name), store_of(hip, name)
    begin(be, name)
    want = export(hip, name)
    assert same_bytes(be.reconstruct_warp(x, y, t), want)
    assert same_bytes(be.reconstruct_warp_aos(_lib.dvs_events(x, y, t)), want)
    assert same_bytes(be.reconstruct_warp_from(store, 0, n), want)
    for dtype, tdt in ((np.float64, torch.float64), (np.float32, torch.float32)):
        d_xy = torch.full((n, 2), -7.0, dtype=tdt, device="cuda")
        d_fl = torch.full((n,), 99, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()  # (the fills run on torch's stream, the export on the context's)
        out = be.reconstruct_warp_from(store, 0, n, dtype=dtype, out=(d_xy, d_fl))
        assert out[0] is d_xy and out[1] is d_fl
        torch.cuda.synchronize()
        assert same_bytes((d_xy.cpu().numpy(), d_fl.cpu().numpy()), be.reconstruct_warp_from(store, 0, n, dtype=dtype))
    # a sub-range that starts and ends off the batch grid, no flags wanted, outputs off the 16-byte grid
    lo, m = 7 * 64 + 1, 5 * 64 + 1
    if n >= lo + m:
        sub = be.reconstruct_warp_from(store, lo, m)
        assert same_bytes(be.reconstruct_warp(x[lo:lo + m], y[lo:lo + m], t[lo:lo + m]), sub)
        buf = torch.full((2 * m + 1,), -7.0, dtype=torch.float64, device="cuda")
        fbuf = torch.full((m + 3,), 99, dtype=torch.uint8, device="cuda")
        xbuf = torch.empty((m, 2), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()  # (the fills run on torch's stream, the export on the context's)
        be.reconstruct_warp_from(store, lo, m, out=(buf[1:], None))
        torch.cuda.synchronize()
        got = buf.cpu().numpy()
        assert got[0] == -7.0 and got[1:].reshape(m, 2).tobytes() == sub[0].tobytes()
        be.reconstruct_warp_from(store, lo, m, out=(xbuf, fbuf[1:m + 1]))
        torch.cuda.synchronize()
        f = fbuf.cpu().numpy()
        assert f[0] == 99 and f[m + 1] == 99 and f[m + 2] == 99 and f[1:m + 1].tobytes() == sub[1].tobytes()
    be.reconstruct_end()
    store.close()


# ---------------------------------------------------------------- 5. slices
def test_internal_slices_change_nothing(hip):
    name = "A"
    _, x, y, t = rc.window(name)
    n = rc.CASES[name]["N"]
    want = export(hip, name)
    be, store = make(hip, name), store_of(hip, name)
    begin(be, name)
    L = _lib.lib()
    try:
        for n_slice in (1000, 4096, 0):
            assert L.cmx_diag_set(_lib.DIAG_RECON_SLICE_EVENTS, n_slice) == 0
            assert same_bytes(be.reconstruct_warp_from(store, 0, n), want), n_slice
            assert same_bytes(be.reconstruct_warp(x, y, t), want), n_slice
            assert same_bytes(be.reconstruct_warp_aos(_lib.dvs_events(x, y, t)), want), n_slice
            assert same_bytes(be.reconstruct_warp(x, y, t, dtype=np.float32), (want[0].astype(np.float32), want[1])), n_slice
    finally:
        assert L.cmx_diag_set(_lib.DIAG_RECON_SLICE_EVENTS, 0) == 0
    be.reconstruct_end()
    store.close()


# ---------------------------------------------------------------- 6. edge counts
def test_edge_counts(hip, oracle):
    # n0: nothing is written
    be = make(hip, "n0")
    begin(be, "n0")
    e = np.zeros(0, np.uint16)
    xy, fl = be.reconstruct_warp(e, e, np.zeros(0, np.int64))
    assert xy.shape == (0, 2) and fl.shape == (0,)
    store = hip.EventStore(W, H, 16)
    assert be.reconstruct_warp_from(store, 0, 0)[0].shape == (0, 2)
    L = _lib.lib()
    guard_xy, guard_fl = np.full(4, -7.0), np.full(4, 99, np.uint8)
    assert L.cmx_backend_recon_warp(be._ctx, 0, None, None, None, _lib.WARP_F64, guard_xy.ctypes.data, guard_fl.ctypes.data) == 0
    assert L.cmx_backend_recon_warp(be._ctx, 0, None, None, None, _lib.WARP_F64, None, None) == 0
    assert (guard_xy == -7.0).all() and (guard_fl == 99).all()
    store.close()
    be.reconstruct_end()
    # n1: the lone event alone -- its own time, not sampled
    for name in ("n1", "n2", "n65"):
        c = rc.CASES[name]
        _, x, y, t = rc.window(name)
        px, py, fl_ref = wc.reference(oracle, name)
        xy, fl = export(hip, name)
        be = make(hip, name)
        begin(be, name)
        host = be.reconstruct_warp(x, y, t)
        nofl = np.empty((c["N"], 2))
        assert L.cmx_backend_recon_warp(be._ctx, c["N"], x.ctypes.data_as(_lib.c_u16p), y.ctypes.data_as(_lib.c_u16p),
                                        t.ctypes.data_as(_lib.c_i64p), _lib.WARP_F64, nofl.ctypes.data, None) == 0
        be.reconstruct_end()
        assert same_bytes(host, (xy, fl)) and nofl.tobytes() == xy.tobytes()
        assert np.abs(xy[:, 0] - px).max() <= PARITY_BOUND and np.abs(xy[:, 1] - py).max() <= PARITY_BOUND
        np.testing.assert_array_equal(fl, fl_ref)
    assert export(hip, "n1")[1][0] & 1 == 0 and export(hip, "n1")[0].shape == (1, 2)
    assert (export(hip, "n2")[1] & 1).all()
    fl = export(hip, "n65")[1]
    assert (fl[:64] & 1).all() and fl[64] & 1 == 0 and fl[64] & 2  # the lone event: a coordinate, inside, not sampled
    # the lone event's pose is the one at ITS time, not the batch's: the reference with the batch pose is far outside the bound
    _, x, y, t = rc.window("n65")
    t_batch = t.copy()
    t_batch[64] = wc.pose_times(t, 64)[0]
    wrong = wc.reference_of(oracle, "n65", x, y, t_batch)
    xy = export(hip, "n65")[0]
    assert abs(xy[64, 0] - wrong[0][64]) > 1e3 * PARITY_BOUND or abs(xy[64, 1] - wrong[1][64]) > 1e3 * PARITY_BOUND
    # batch5000: a batch spans several workgroups; B at rate 3: unsampled events carry coordinates and clear bit 0
    fl = export(hip, "batch5000")[1]
    assert (fl & 1).all()
    xy, fl = export(hip, "B")
    i = np.arange(30_001)
    assert np.array_equal((fl & 1).astype(bool), (i % 64) % 3 == 0)  # (30 001 = 468 x 64 + 49: no lone event)
    assert np.isfinite(xy).all() and (fl[(fl & 1) == 0] & 2).any()


# ---------------------------------------------------------------- 7. read-only
def test_the_export_changes_nothing(hip, oracle):
    name = "window"
    c, (w, x, y, t) = rc.CASES[name], rc.window(name)
    n = c["N"]
    be, store = make(hip, name, deterministic=True), store_of(hip, name)
    zero = np.zeros(3 * c["K"])
    be.set_window(x[:5000], y[:5000], t[:5000], c["order"], w.knots_true, w.start_ns, w.dt_ns, 0, 2 ** 62, c["batch"], c["rate"])
    win_before = be.eval(zero)
    begin(be, name)
    first = be.reconstruct_warp_from(store, 0, n)
    # an open gradient pass with half of its events added
    be.reconstruct_add_from(store, 0, n)
    be.reconstruct_contrast(1.0, want_grad=True)
    be.reconstruct_grad_add_from(store, 0, 10_000)
    state = be.reconstruct_get(with_counts=True)
    assert same_bytes(be.reconstruct_warp_from(store, 0, n), first)
    assert same_bytes(be.reconstruct_warp(x, y, t), first)
    be.reconstruct_grad_add_from(store, 10_000, n - 10_000)
    grad = be.reconstruct_grad_get()  # (CMX_ERR_STATE had the export closed the pass or touched its counts)
    assert np.abs(grad).max() > 0
    be.reconstruct_warp_from(store, 0, n)
    assert be.reconstruct_grad_get().tobytes() == grad.tobytes()
    now = be.reconstruct_get(with_counts=True)
    assert now[0].tobytes() == state[0].tobytes() and now[1:] == state[1:]
    # the same sums from a run without any export in between
    ref = make(hip, name, deterministic=True)
    begin(ref, name)
    ref.reconstruct_add_from(store, 0, n)
    ref.reconstruct_contrast(1.0, want_grad=True)
    ref.reconstruct_grad_add_from(store, 0, 10_000)
    ref.reconstruct_grad_add_from(store, 10_000, n - 10_000)
    assert ref.reconstruct_grad_get().tobytes() == grad.tobytes()
    ref.reconstruct_end()
    # a binding with a frozen head
    be.reconstruct_bind(store, 0, n)
    be.reconstruct_freeze_head(5)
    ev = be.reconstruct_eval_bound(None, 1.0)
    infos = (be.reconstruct_bound_info(), be.reconstruct_frozen_info(), be.reconstruct_online_info())
    assert infos[1]["frozen_batches"] > 0
    state = be.reconstruct_get(with_counts=True)
    assert same_bytes(be.reconstruct_warp_from(store, 0, n), first)
    assert (be.reconstruct_bound_info(), be.reconstruct_frozen_info(), be.reconstruct_online_info()) == infos
    now = be.reconstruct_get(with_counts=True)
    assert now[0].tobytes() == state[0].tobytes() and now[1:] == state[1:]
    ev2 = be.reconstruct_eval_bound(None, 1.0)
    assert ev2[0] == ev[0] and ev2[1].tobytes() == ev[1].tobytes()
    assert be.reconstruct_bound_info()["sorts"] == infos[0]["sorts"]  # (the tile sort survived)
    # after release_head restart is refused; the export reads only the knots
    be.reconstruct_release_head()
    on = be.reconstruct_online_info()
    assert on["released_sampled"] > 0
    assert status_of(hip, be.reconstruct_restart, w.knots_true) == _lib.ERR_STATE
    assert same_bytes(be.reconstruct_warp_from(store, 0, n), first)
    assert be.reconstruct_online_info() == on
    # the window evaluation is where it was
    win_after = be.eval(zero)
    assert win_after[0] == win_before[0] and win_after[1].tobytes() == win_before[1].tobytes()
    be.reconstruct_end()
    # it tracks the knots: after restart(knots2) the export is the reference at knots2
    knots2 = synth.backend_window(200, W, H, *rc.SENSOR[2:], c["Wp"], c["Hp"], c["order"], c["K"], 0, (c["K"] - c["order"] + 1) * rc.DT,
                                  dt_knots=rc.DT, seed=99).knots_true
    assert np.abs(knots2 - w.knots_true).max() > 1e-3
    begin(be, name)
    be.reconstruct_restart(knots2)
    xy, fl = be.reconstruct_warp_from(store, 0, n)
    be.reconstruct_end()
    store.close()
    px, py, fl_ref = wc.reference_of(oracle, name, x, y, t, knots=knots2)
    print("parity window at other knots: max|px - ref| %.3e  max|py - ref| %.3e" % (np.abs(xy[:, 0] - px).max(), np.abs(xy[:, 1] - py).max()))
    assert np.abs(xy[:, 0] - px).max() <= PARITY_BOUND and np.abs(xy[:, 1] - py).max() <= PARITY_BOUND
    keep = ~wc.near_integer(px, py)
    assert np.count_nonzero(~keep) <= wc.MAX_NEAR_INTEGER
    np.testing.assert_array_equal(fl[keep], fl_ref[keep])
    assert np.abs(xy - first[0]).max() > 0.1  # (another trajectory: the coordinates moved, by pixels)


# ---------------------------------------------------------------- 8. errors
def test_errors_write_nothing(hip):
    name = "window"
    c, (w, x, y, t) = rc.CASES[name], rc.window(name)
    n = c["N"]
    L = _lib.lib()
    be = make(hip, name)
    xy, fl = np.full((n + 1, 2), -7.0), np.full(n + 1, 99, np.uint8)

    def raw(ctx, x, y, t, fmt=_lib.WARP_F64, xy_ptr=None, count=None):
        return L.cmx_backend_recon_warp(ctx, len(x) if count is None else count, x.ctypes.data_as(_lib.c_u16p), y.ctypes.data_as(_lib.c_u16p),
                                        t.ctypes.data_as(_lib.c_i64p), fmt, xy.ctypes.data if xy_ptr is None else xy_ptr, fl.ctypes.data)

    def raw_from(ctx, store, first, count, fmt=_lib.WARP_F64):
        return L.cmx_backend_recon_warp_from(ctx, store._h, first, count, fmt, xy.ctypes.data, fl.ctypes.data)

    def untouched():
        assert (xy == -7.0).all() and (fl == 99).all()

    store = store_of(hip, name)
    # before begin, and on a group handle
    assert raw(be._ctx, x, y, t) == _lib.ERR_STATE
    assert raw_from(be._ctx, store, 0, n) == _lib.ERR_STATE
    assert status_of(hip, be.reconstruct_warp_aos, _lib.dvs_events(x, y, t)) == _lib.ERR_STATE
    grp = hip.BackendEvaluator(W, H, w.lut, c["Wp"], c["Hp"], devices=[0, 0], transport=_lib.GROUP_DIRECT)
    assert raw(grp._ctx, x, y, t) == _lib.ERR_STATE
    assert status_of(hip, grp.reconstruct_warp, x, y, t) == _lib.ERR_STATE
    grp.close()
    untouched()
    begin(be, name)
    # format and output pointer
    assert raw(be._ctx, x, y, t, fmt=2) == _lib.ERR_INVALID_ARG
    assert raw(be._ctx, x, y, t, fmt=-1) == _lib.ERR_INVALID_ARG
    assert raw_from(be._ctx, store, 0, n, fmt=7) == _lib.ERR_INVALID_ARG
    assert L.cmx_backend_recon_warp(be._ctx, n, x.ctypes.data_as(_lib.c_u16p), y.ctypes.data_as(_lib.c_u16p), t.ctypes.data_as(_lib.c_i64p),
                                    _lib.WARP_F64, None, fl.ctypes.data) == _lib.ERR_INVALID_ARG
    assert L.cmx_backend_recon_warp_from_device(be._ctx, store._h, 0, n, _lib.WARP_F64, None, None) == _lib.ERR_INVALID_ARG
    assert raw_from(be._ctx, store, 0, n + 1) == _lib.ERR_INVALID_ARG
    assert raw(be._ctx, x, y, t, count=-1) == _lib.ERR_INVALID_ARG
    untouched()
    # an event outside the sensor near the end: an unsampled one counts too
    bad_x = x.copy()
    bad_x[-2] = W
    assert raw(be._ctx, bad_x, y, t) == _lib.ERR_EVENT_RANGE
    bad_y = y.copy()
    bad_y[-2] = H
    assert status_of(hip, be.reconstruct_warp_aos, _lib.dvs_events(x, bad_y, t)) == _lib.ERR_EVENT_RANGE
    untouched()
    # a batch whose first event is later than its last one
    back = t.copy()
    back[19_900] = t[19_999] + 1000
    assert raw(be._ctx, x, y, back) == _lib.ERR_TIME_ORDER
    st = hip.EventStore(W, H, n)
    st.push(x, y, back)
    assert raw_from(be._ctx, st, 0, n) == _lib.ERR_TIME_ORDER
    st.close()
    untouched()
    # batch times outside the spline: the last two batches alone
    only_tail = t.copy()
    only_tail[-150:] += 10_000_000_000
    assert raw(be._ctx, x, y, only_tail) == _lib.ERR_SPLINE_RANGE
    st = hip.EventStore(W, H, n + 1)
    st.push(x, y, only_tail)
    assert raw_from(be._ctx, st, 0, n) == _lib.ERR_SPLINE_RANGE
    st.close()
    untouched()
    # the lone trailing event outside the spline: add* skips it, the export refuses it
    x1, y1 = np.append(x, x[-1]), np.append(y, y[-1])
    t1 = np.append(t, t[-1] + 10_000_000_000)
    assert n % c["batch"] == 0
    be.reconstruct_add(x1, y1, t1)
    assert raw(be._ctx, x1, y1, t1) == _lib.ERR_SPLINE_RANGE
    st = hip.EventStore(W, H, n + 1)
    st.push(x1, y1, t1)
    assert raw_from(be._ctx, st, 0, n + 1) == _lib.ERR_SPLINE_RANGE
    assert raw_from(be._ctx, st, n, 1) == _lib.ERR_SPLINE_RANGE
    assert raw(be._ctx, x1[n:], y1[n:], t1[n:]) == _lib.ERR_SPLINE_RANGE
    untouched()
    # ... and the same input without that event is fine, which the guards show as written
    assert raw_from(be._ctx, st, 0, n) == 0
    st.close()
    assert (xy[:n] != -7.0).all() and (xy[n] == -7.0).all() and (fl[:n] <= 3).all() and fl[n] == 99
    be.reconstruct_end()
    store.close()


# ---------------------------------------------------------------- 9. example
def test_example_exports_the_warped_events(hip, tmp_path):
    ex = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples")
    if ex not in sys.path:
        sys.path.insert(0, ex)
    import rotation_pipeline as rp
    stream = synth.event_stream(2e6, 0.5, 240, 180, 200.0, 200.0, 119.5, 89.5, omega_mean=(0.2, 1.8, 0.3), omega_amp=(1.0, 0.8, 1.0), seed=77)
    path = str(tmp_path / "warped")
    res = rp.run_pipeline(stream, rp.Params(), export_warped=path)
    z = np.load(path + ".npz")
    xy, fl, index = z["xy"], z["flags"], z["index"]
    n = len(index)
    assert xy.shape == (n, 2) and xy.dtype == np.float64 and fl.shape == (n,) and fl.dtype == np.uint8
    assert n > 0.5 * len(stream.t_ns) and np.array_equal(index, np.arange(index[0], index[0] + n))
    Hp, Wp = res["recon"].shape
    r = rel_img(wc.revote(xy[:, 0], xy[:, 1], fl, Hp, Wp), res["recon"])
    print("example: %d events exported, %d voted; host re-vote vs the example's panorama %.2e" % (n, np.count_nonzero(fl == 3), r))
    assert r < RTOL
    ap_help = open(os.path.join(ex, "rotation_pipeline.py")).read()
    assert "--export-warped" in ap_help
