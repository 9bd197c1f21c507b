"""-m gpu: cmx_events_select[_device], cmx_events_pixel_counts[_device] and cmx_events_read -- the stable device-side compaction of
a range of one event store into another, the per-pixel histogram and the read-back.

Everything is integers or one fp32 compare, so EVERY comparison is exact: EventStore.read of the destination against
events_select_cases.compact under events_select_cases.predicate of the pushed arrays; consumers fed from a selected store against
the same consumers fed from a store the numpy-compacted arrays were pushed into, bitwise, in deterministic mode."""
import numpy as np
import pytest

import events_select_cases as ec
import recon_cases as rc
from cmax_slam_amd import _lib

pytestmark = pytest.mark.gpu
W, H = ec.W, ec.H


def same_events(a, b):
    """(x, y, t, pol or None) tuples, element for element and type for type"""
    for p, q in zip(a, b):
        if (p is None) != (q is None):
            return False
        if p is not None and (np.asarray(p).shape != np.asarray(q).shape or np.asarray(p).tobytes() != np.asarray(q, np.asarray(p).dtype).tobytes()):
            return False
    return len(a) == len(b)


def pushed(hip, arrays, capacity=None):
    x, y, t, pol = arrays
    store = hip.EventStore(W, H, max(capacity if capacity is not None else len(x), 1))
    if len(x):
        store.push(x, y, t, pol)
    return store


def whole(store):
    return store.read(store.begin, store.end - store.begin)


def status_of(hip, fn, *a, **k):
    with pytest.raises(hip.CmaxHipError) as e:
        fn(*a, **k)
    return e.value.status


def recon_of(hip, store, first, count, deterministic=True):
    """(plane bytes, n_sampled, n_inside) of the "window" configuration's reconstruction over store[first, first + count): a consumer
    that forms its batch times on the host, from the store's mirror of the timestamps"""
    w = rc.window("window")[0]
    c = rc.CASES["window"]
    be = hip.BackendEvaluator(W, H, w.lut, c["Wp"], c["Hp"])
    be.set_deterministic(deterministic)
    be.reconstruct_begin(c["order"], w.knots_true, w.start_ns, w.dt_ns, c["batch"], c["rate"])
    be.reconstruct_add_from(store, first, count)
    plane, ns, ni = be.reconstruct_get(with_counts=True)
    be.reconstruct_end()
    assert ni > 0
    return plane.tobytes(), ns, ni


def window_arrays():
    x, y, t = rc.window("window")[1:]
    return x, y, t, None


def on_device(sel):
    import torch
    out = {k: (torch.from_numpy(np.array(v)).cuda() if isinstance(v, np.ndarray) else v) for k, v in sel.items()}
    torch.cuda.synchronize()  # (the copies run on torch's stream, the selection on the store's)
    return out


@pytest.fixture(scope="module")
def base(hip):
    """the base stream (read-only) and two source stores holding it, with and without polarity"""
    x, y, t, pol = ec.stream()[:4]
    return dict(arrays=(x, y, t, pol), pol=pushed(hip, (x, y, t, pol)), nopol=pushed(hip, (x, y, t, None)))


def check_select(hip, src, arrays, first, count, sel, device=False, dst=None, before=None):
    """select src[first, first+count) into dst (a fresh store by default) and compare all of dst with `before` + the compaction"""
    x, y, t, pol = arrays
    lo = first - src.begin
    sl = slice(lo, lo + count)
    keep = ec.predicate(sel, x[sl], y[sl], W)
    if dst is None:
        dst = hip.EventStore(W, H, max(count, 1))
    b0, e0 = dst.begin, dst.end
    n = dst.select(src, first, count, **(on_device(sel) if device else sel))
    assert n == int(keep.sum())
    assert (dst.begin, dst.end) == (b0, e0 + n)
    want = ec.compact((x[sl], y[sl], t[sl], pol[sl] if pol is not None else None), keep)
    if before is not None:
        want = tuple(None if w is None else np.concatenate([p, w]) for p, w in zip(before, want))
    if dst.end == dst.begin:
        want = want[:3] + (None,)  # (an empty store has no polarity form)
    got = whole(dst)
    assert same_events(got, want)
    assert dst.has_polarity == (pol is not None and dst.end > dst.begin)
    return dst, keep


# ---------------------------------------------------------------- counts: every wave and tile edge
@pytest.mark.parametrize("count", ec.COUNTS)
def test_counts(hip, base, count):
    check_select(hip, base["pol"], base["arrays"], 0, count, dict(keep=ec.random_keep(count, count)))


def test_more_tiles_than_one_scan_pass(hip, base):
    x, y, t, pol = base["arrays"]
    reps = -(-ec.N_SCAN // len(x))
    span = int(t[-1] - t[0]) + 1
    big = (np.tile(x, reps)[:ec.N_SCAN], np.tile(y, reps)[:ec.N_SCAN],
           np.concatenate([t + k * span for k in range(reps)])[:ec.N_SCAN], np.tile(pol, reps)[:ec.N_SCAN])
    src = pushed(hip, big)
    keep = ec.random_keep(ec.N_SCAN, 99)
    keep[-1] = 1  # (the one event of the last tile, behind a full pass of the scan)
    check_select(hip, src, big, 0, ec.N_SCAN, dict(keep=keep))


# ---------------------------------------------------------------- patterns
@pytest.mark.parametrize("name", list(ec.PATTERNS))
def test_patterns(hip, base, name):
    kind, sel, keep = ec.kept_of_case(ec.PATTERNS, name, ec.N_BIG)
    dst, got = check_select(hip, base["nopol"], base["arrays"][:3] + (None,), 0, ec.N_BIG, sel)
    assert (got == keep).all() and dst.end == int(keep.sum())


# ---------------------------------------------------------------- offsets
@pytest.mark.parametrize("first", [1, 67])
@pytest.mark.parametrize("held", [0, 1, 129])
def test_unaligned_source_and_destination(hip, base, first, held):
    x, y, t, pol = base["arrays"]
    early = (x[:held], y[:held], np.minimum(t[:held], t[first]), pol[:held])  # (no later than the first event selected below)
    dst = pushed(hip, early, capacity=held + ec.N_BIG)
    check_select(hip, base["pol"], base["arrays"], first, ec.N_BIG, dict(keep=ec.random_keep(ec.N_BIG, first)), dst=dst, before=early)


def test_source_after_drop_before(hip, base):
    arrays = base["arrays"]
    src = pushed(hip, arrays)
    src.drop_before(1000 + 3)  # first_index != 0, and the second buffer is the current one
    assert src.begin == 1003
    check_select(hip, src, tuple(a[1003:] for a in arrays), 1003 + 5, 9000, dict(keep=ec.random_keep(9000, 5)))
    src.drop_before(2000 + 1)  # ... and the first one again
    check_select(hip, src, tuple(a[2001:] for a in arrays), 2001, 4097, dict(keep=ec.random_keep(4097, 6)))


def test_destination_dropped_then_appended(hip):
    arrays = window_arrays()
    src = pushed(hip, arrays)
    k1 = ec.random_keep(8_000, 11)
    dst, keep1 = check_select(hip, src, arrays, 0, 8_000, dict(keep=k1), dst=hip.EventStore(W, H, 40_000))
    n1 = int(keep1.sum())
    dst.drop_before(777)
    assert (dst.begin, dst.end) == (777, n1)
    left = tuple(None if a is None else a[777:] for a in ec.compact(tuple(None if a is None else a[:8_000] for a in arrays), keep1))
    assert same_events(whole(dst), left)
    dst, keep2 = check_select(hip, src, arrays, 8_000, 12_000, dict(keep=ec.random_keep(12_000, 12)), dst=dst, before=left)
    # the host mirror of the timestamps went along with the drop and the append: a consumer that forms its batch times from it gives
    # the bits it gives on a store the same events were pushed into, over the whole store and over a range across the joint
    twin = pushed(hip, whole(dst))
    n = dst.end - dst.begin
    assert n == n1 - 777 + int(keep2.sum()) and (twin.begin, twin.end) == (0, n)
    assert recon_of(hip, dst, dst.begin, n) == recon_of(hip, twin, 0, n)
    cut = n1 - 777 - 1234
    assert recon_of(hip, dst, dst.begin + cut, 5_001) == recon_of(hip, twin, cut, 5_001)


# ---------------------------------------------------------------- criteria, both polarity forms, both argument forms
@pytest.mark.parametrize("with_pol", [False, True])
@pytest.mark.parametrize("name", list(ec.CRITERIA))
def test_criteria_host_and_device_forms(hip, base, name, with_pol):
    kind, sel, keep = ec.kept_of_case(ec.CRITERIA, name, ec.N_CRIT)
    src = base["pol" if with_pol else "nopol"]
    arrays = base["arrays"] if with_pol else base["arrays"][:3] + (None,)
    host, got = check_select(hip, src, arrays, 0, ec.N_CRIT, sel)
    assert (got == keep).all()
    dev, _ = check_select(hip, src, arrays, 0, ec.N_CRIT, sel, device=True)
    assert same_events(whole(host), whole(dev))
    if name == "pixel":
        is_hot = ec.stream()[4][:ec.N_CRIT]
        assert not (keep & is_hot).any() and int((~keep).sum()) >= int(is_hot.sum()) > 0


def test_python_argument_checks(hip, base):
    import torch
    src, dst = base["nopol"], hip.EventStore(W, H, 100)
    k = np.ones(50, np.uint8)
    with pytest.raises(ValueError):
        dst.select(src, 0, 50, keep=k, flags=torch.zeros(50, dtype=torch.uint8, device="cuda"))  # mixed
    with pytest.raises(ValueError):
        dst.select(src, 0, 50, score=np.zeros(50, np.float32))
    with pytest.raises(ValueError):
        dst.select(src, 0, 50, min_score=1.0)
    with pytest.raises(ValueError):
        dst.select(src, 0, 50, keep=k[:49])
    with pytest.raises(ValueError):
        dst.select(src, 0, 50, pixel_keep=np.ones((H, W - 1), np.uint8))
    with pytest.raises(ValueError):
        dst.select(src, 0, 50, keep=torch.zeros(50, dtype=torch.float32, device="cuda"))
    with pytest.raises(ValueError):
        dst.select(src, 0, 50, keep=torch.ones(50, dtype=torch.uint8))  # a tensor in host memory is no device pointer
    with pytest.raises(ValueError):
        src.pixel_counts(0, 50, out=torch.zeros((H, W), dtype=torch.int32))
    assert (dst.begin, dst.end) == (0, 0)
    assert dst.select(src, 0, 50, keep=k.astype(bool)) == 50


# ---------------------------------------------------------------- pixel_counts
def bincount(x, y):
    return np.bincount(y.astype(np.int64) * W + x.astype(np.int64), minlength=W * H).reshape(H, W).astype(np.uint32)


def test_pixel_counts(hip, base):
    import torch
    x, y, t, pol = base["arrays"]
    store = base["pol"]
    for first, count in ((0, len(x)), (67, 20_001), (5, 0), (len(x), 0)):
        want = bincount(x[first:first + count], y[first:first + count])
        got = store.pixel_counts(first, count)
        assert got.dtype == np.uint32 and got.shape == (H, W) and got.tobytes() == want.tobytes()
        out = torch.full((H, W), 12345, dtype=torch.int32, device="cuda")  # (written, not accumulated)
        torch.cuda.synchronize()
        assert store.pixel_counts(first, count, out=out) is out
        assert out.cpu().numpy().view(np.uint32).tobytes() == want.tobytes()
    hot = ec.stream()[5]
    assert store.pixel_counts(0, len(x))[hot[0, 1], hot[0, 0]] > 100
    assert status_of(hip, store.pixel_counts, 1, len(x)) == _lib.ERR_INVALID_ARG


def test_pixel_counts_with_one_pixel_above_16_bits(hip):
    rng = np.random.default_rng(8)
    n, n_hot = 100_000, 70_000
    x = rng.integers(0, W, n).astype(np.uint16)
    y = rng.integers(0, H, n).astype(np.uint16)
    at = rng.permutation(n)[:n_hot]
    x[at], y[at] = 17, 3
    t = np.sort(rng.integers(0, 10**9, n)).astype(np.int64)
    store = pushed(hip, (x, y, t, None))
    got = store.pixel_counts(0, n)
    assert got[3, 17] >= n_hot > 65_535 and got.tobytes() == bincount(x, y).tobytes()


# ---------------------------------------------------------------- read
@pytest.mark.parametrize("with_pol", [False, True])
def test_read_round_trip(hip, base, with_pol):
    x, y, t, pol = base["arrays"]
    store = base["pol" if with_pol else "nopol"]
    for first, count in ((0, len(x)), (1, 4097), (len(x) - 3, 3), (9, 0)):
        sl = slice(first, first + count)
        got = store.read(first, count)
        assert [a.dtype for a in got[:3]] == [np.uint16, np.uint16, np.int64]
        assert same_events(got, (x[sl], y[sl], t[sl], pol[sl] if with_pol else None))
    assert status_of(hip, store.read, 0, len(x) + 1) == _lib.ERR_INVALID_ARG
    if not with_pol:  # asking a store without polarity for it
        p = np.zeros(4, np.uint8)
        rc_ = _lib.lib().cmx_events_read(store._h, 0, 4, None, None, None, p.ctypes.data_as(_lib.c_u8p))
        assert rc_ == _lib.ERR_STATE
    else:  # any of x, y, t may be NULL
        p = np.zeros(70, np.uint8)
        yy = np.zeros(70, np.uint16)
        assert _lib.lib().cmx_events_read(store._h, 3, 70, None, yy.ctypes.data_as(_lib.c_u16p), None, p.ctypes.data_as(_lib.c_u8p)) == 0
        assert (yy == y[3:73]).all() and (p == pol[3:73]).all()


def test_read_spans_two_staging_slices(hip):
    """two pushes of fewer than 2^16 events each leave the pinned staging at its smallest size, 2^16 events; together they hold
    more, so a read of the whole store takes two slices"""
    n1, n2 = 40_000, 39_857
    n = n1 + n2
    assert n1 < (1 << 16) and n2 < (1 << 16) and n > (1 << 16)
    rng = np.random.default_rng(9)
    arrays = (rng.integers(0, W, n).astype(np.uint16), rng.integers(0, H, n).astype(np.uint16),
              np.sort(rng.integers(0, 10**12, n)).astype(np.int64), rng.integers(0, 2, n).astype(np.uint8))
    store = hip.EventStore(W, H, n)
    store.push(*(a[:n1] for a in arrays))
    store.push(*(a[n1:] for a in arrays))
    assert same_events(whole(store), arrays)
    assert same_events(store.read(12_345, 60_000), tuple(a[12_345:72_345] for a in arrays))  # (fits one slice)
    assert same_events(store.read(1, n - 1), tuple(a[1:] for a in arrays))
    dst = hip.EventStore(W, H, n)  # no push at all: the selection allocates the staging
    assert dst.select(store, 0, n) == n  # no criterion: a device-side copy
    assert same_events(whole(dst), arrays) and same_events(whole(store), arrays)


@pytest.mark.parametrize("n_slice", [1000, 4096, 1])
def test_select_read_back_and_read_in_slices(hip, n_slice):
    """CMX_DIAG_EVENTS_STAGE_SLICE: the timestamps' read-back of a selection and cmx_events_read in slices of n_slice events -- the
    appends to the host mirror at every offset, after a time-order refusal in the FIRST slice, behind events that were pushed"""
    L = _lib.lib()
    arrays = window_arrays()
    x, y, t, _ = arrays
    n = len(x) if n_slice > 1 else 300  # (one event per slice: a few hundred round trips are enough)
    held = 3_000 if n_slice > 1 else 50
    src = pushed(hip, arrays)
    dst = pushed(hip, tuple(None if a is None else a[:held] for a in arrays), capacity=n)
    keep = ec.random_keep(n - held, 31)
    want = tuple(None if a is None else np.concatenate([a[:held], a[held:n][keep != 0]]) for a in arrays)
    try:
        assert L.cmx_diag_set(_lib.DIAG_EVENTS_STAGE_SLICE, n_slice) == 0
        assert int(keep.sum()) > 2 * n_slice
        assert status_of(hip, dst.select, src, held - 10, 100) == _lib.ERR_TIME_ORDER and (dst.begin, dst.end) == (0, held)
        assert dst.select(src, held, n - held, keep=keep) == int(keep.sum())
        assert same_events(whole(dst), want)  # (read in slices too)
        assert same_events(dst.read(7, n_slice + 3), tuple(None if a is None else a[7:n_slice + 10] for a in want))
    finally:
        assert L.cmx_diag_set(_lib.DIAG_EVENTS_STAGE_SLICE, 0) == 0
    assert L.cmx_diag_set(_lib.DIAG_EVENTS_STAGE_SLICE, -1) != 0
    assert same_events(whole(dst), want)
    if n_slice > 1:  # the mirror the slices appended to is the one a push of the same events builds
        twin = pushed(hip, want)
        m = dst.end - dst.begin
        assert recon_of(hip, dst, 0, m) == recon_of(hip, twin, 0, m)
        assert recon_of(hip, dst, held - 500, 4_321) == recon_of(hip, twin, held - 500, 4_321)


# ---------------------------------------------------------------- consumers: a selected store is an ordinary store
@pytest.fixture(scope="module")
def twins(hip):
    """the "window" configuration, half of it kept at random: (window, kept arrays, store filled by select, store filled by push)"""
    w, x, y, t = rc.window("window")
    keep = ec.random_keep(len(x), 21)
    src = pushed(hip, (x, y, t, None))
    a = hip.EventStore(W, H, len(x))
    assert a.select(src, 0, len(x), keep=keep) == int(keep.sum())
    kept = ec.compact((x, y, t), keep.astype(bool))
    b = pushed(hip, kept + (None,))
    return w, kept, a, b


def test_consumer_reconstruct_add_from(hip, twins):
    w, kept, a, b = twins
    c = rc.CASES["window"]
    out = []
    for store in (a, b):
        be = hip.BackendEvaluator(W, H, w.lut, c["Wp"], c["Hp"])
        be.set_deterministic(True)
        be.reconstruct_begin(c["order"], w.knots_true, w.start_ns, w.dt_ns, c["batch"], c["rate"])
        be.reconstruct_add_from(store, 0, len(kept[0]))
        out.append(be.reconstruct_get(with_counts=True))
        be.reconstruct_end()
    assert float(out[0][0].max()) > 0 and out[0][0].tobytes() == out[1][0].tobytes() and out[0][1:] == out[1][1:]
    assert out[0][1] == rc.sampled(len(kept[0]), c["batch"], c["rate"])


def test_consumer_bound_evaluation(hip, twins):
    w, kept, a, b = twins
    c = rc.CASES["window"]
    out = []
    for store in (a, b):
        be = hip.BackendEvaluator(W, H, w.lut, c["Wp"], c["Hp"])
        be.set_deterministic(True)
        be.reconstruct_begin(c["order"], w.knots_true, w.start_ns, w.dt_ns, c["batch"], c["rate"])
        be.reconstruct_bind(store, 0, len(kept[0]))
        out.append(be.reconstruct_eval_bound(None, 1.0))
        be.reconstruct_end()
    assert out[0][0] > 0 and np.abs(out[0][1]).max() > 0
    assert out[0][0] == out[1][0] and np.asarray(out[0][1]).tobytes() == np.asarray(out[1][1]).tobytes()


def test_consumer_frontend_packet(hip, twins):
    w, kept, a, b = twins
    fx, fy, cx, cy = rc.SENSOR[2:]
    first, n = 100, 6000
    t_ref = int(kept[2][first + n // 2])
    out = []
    for store in (a, b):
        fe = hip.FrontendEvaluator(W, H, w.lut)
        fe.set_deterministic(True)
        fe.set_packet_from(store, first, n, t_ref, fx, fy, cx, cy)
        out.append(fe.eval((0.3, -0.5, 0.2)))
    assert out[0][0] > 0 and out[0][0] == out[1][0] and np.asarray(out[0][1]).tobytes() == np.asarray(out[1][1]).tobytes()


# ---------------------------------------------------------------- the loop it is for
def test_reject_by_score_on_the_device(hip):
    import torch
    name = "window"
    c = rc.CASES[name]
    w, x, y, t = rc.window(name)
    n = len(x)
    src = pushed(hip, (x, y, t, None))
    be = hip.BackendEvaluator(W, H, w.lut, c["Wp"], c["Hp"])
    be.reconstruct_begin(c["order"], w.knots_true, w.start_ns, w.dt_ns, c["batch"], c["rate"])
    be.reconstruct_add_from(src, 0, n)
    be.reconstruct_score_open(1.0)
    d_s = torch.empty(n, dtype=torch.float32, device="cuda")
    d_f = torch.empty(n, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    be.reconstruct_score_from(src, 0, n, out=(d_s, d_f))
    s, f = d_s.cpu().numpy(), d_f.cpu().numpy()
    thr = float(np.median(s))
    dst = hip.EventStore(W, H, n)
    kept = dst.select(src, 0, n, score=d_s, min_score=thr, flags=d_f)
    keep = ec.predicate(dict(score=s, min_score=thr, flags=f), x, y, W)
    assert 0 < kept == int(keep.sum()) < n
    assert same_events(whole(dst), ec.compact((x, y, t, None), keep))
    be.reconstruct_end()


def test_example_rejects_outliers(hip):
    """rotation_pipeline.py --reject-outliers [--hot-pixels]: runs, and what it reports is consistent (nothing about quality)"""
    import os
    import sys
    from cmax_slam_amd import synth
    ex = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples")
    if ex not in sys.path:
        sys.path.insert(0, ex)
    import rotation_pipeline as rp
    stream = synth.event_stream(2e6, 0.5, 240, 180, 200.0, 200.0, 119.5, 89.5, omega_mean=(0.2, 1.8, 0.3), omega_amp=(1.0, 0.8, 1.0), seed=77,
                                hot_pixels=2, hot_share=0.04)
    lines = []
    res = rp.run_pipeline(stream, rp.Params(), reject_outliers=1.0, refine_native=True, log=lines.append)
    r = res["reject"]
    assert 0 < r["kept"] <= len(stream.t_ns) and r["share"] <= 1.0
    assert r["recon"].shape == res["recon"].shape and float(r["recon"].sum(dtype=np.float64)) > 0
    assert r["contrast_before"] > 0 and r["contrast_after"] > 0
    assert r["hot_removed"] == 1.0  # (the mask is made from pixel_counts: a pixel with 2 % of the events is 860 times the mean)
    assert 0.0 <= r["hot_removed_by_score"] <= 1.0 and 0.0 < r["others_kept"] <= 1.0
    # with refine_native the trajectory is solved again on the cleaned store
    assert np.asarray(r["knots"]).shape == np.asarray(res["traj"].knots).shape and np.isfinite(r["knots"]).all()
    assert r["report"]["events"] == r["kept"] and r["report"]["contrast_after"] >= r["report"]["contrast_before"] > 0
    assert any("refinement on the cleaned store" in s for s in lines)
    assert any(s.startswith("outlier rejection:") for s in lines) and any("hot pixels:" in s for s in lines)
    src = open(os.path.join(ex, "rotation_pipeline.py")).read()
    assert "--reject-outliers" in src and "--hot-pixels" in src


# ---------------------------------------------------------------- errors: each leaves dst exactly as it was
def test_errors_leave_the_destination_alone(hip, base):
    x, y, t, pol = base["arrays"]
    src_pol, src_nopol = base["pol"], base["nopol"]
    L = _lib.lib()
    held = (x[5000:5100], y[5000:5100], t[5000:5100], None)
    dst = pushed(hip, held, capacity=200)

    def unchanged():
        return (dst.begin, dst.end) == (0, 100) and same_events(whole(dst), held) and not dst.has_polarity

    inv, state, order = _lib.ERR_INVALID_ARG, _lib.ERR_STATE, _lib.ERR_TIME_ORDER
    # a null store, the same store, sel NULL, a foreign size
    sel = _lib.Select(_lib.C.sizeof(_lib.Select))
    n_kept = _lib.C.c_int64(-1)
    for fn in (L.cmx_events_select, L.cmx_events_select_device):
        assert fn(dst._h, None, 0, 10, _lib.C.byref(sel), None) == inv
        assert fn(None, src_nopol._h, 0, 10, _lib.C.byref(sel), None) == inv
        assert fn(dst._h, dst._h, 0, 10, _lib.C.byref(sel), None) == inv
        assert fn(dst._h, src_nopol._h, 6000, 10, None, None) == inv
        bad = _lib.Select(_lib.C.sizeof(_lib.Select) - 8)
        assert fn(dst._h, src_nopol._h, 6000, 10, _lib.C.byref(bad), _lib.C.byref(n_kept)) == inv
        assert unchanged()
    # another sensor
    other = hip.EventStore(W + 1, H, 10)
    other.push(x[:5], y[:5], t[:5])
    assert status_of(hip, dst.select, other, 0, 5) == inv and unchanged()
    # ranges the source does not hold
    n = len(x)
    for first, count in ((-1, 5), (0, n + 1), (n, 1), (10, -1)):
        assert status_of(hip, dst.select, src_nopol, first, count) == inv and unchanged()
    # polarity form
    assert status_of(hip, dst.select, src_pol, 6000, 10) == state and unchanged()
    # time order: the first KEPT event decides
    assert status_of(hip, dst.select, src_nopol, 4000, 50) == order and unchanged()
    k = np.zeros(1200, np.uint8)
    k[1150:1160] = 1  # source events 5150..5159: later than everything held
    k[3] = 1          # ... but 4003 is kept too, and is earlier
    assert t[4003] < t[5099]
    assert status_of(hip, dst.select, src_nopol, 4000, 1200, keep=k) == order and unchanged()
    # capacity: one event too small (100 held + 101 kept > 200)
    k = np.zeros(1200, np.uint8)
    k[1099:1200] = 1
    assert int(k.sum()) == 101 and t[4000 + 1099] >= t[5099]
    e = status_of(hip, dst.select, src_nopol, 4000, 1200, keep=k)
    assert e == inv and b"full" in L.cmx_events_last_error(dst._h) and unchanged()
    # group stores (two replicas need two devices; one device makes a one-replica "group", which is allowed)
    if L.cmx_device_count() >= 2:
        grp = hip.EventStore(W, H, 100, devices=[0, 1])
        assert status_of(hip, grp.select, src_nopol, 0, 10) == inv and b"group" in L.cmx_events_last_error(grp._h)
        assert status_of(hip, dst.select, hip.EventStore(W, H, 10, device=1), 0, 0) == inv and unchanged()
    # and after all of that the store still works: exactly the room that is left
    k[1099] = 0
    assert dst.select(src_nopol, 4000, 1200, keep=k) == 100 and (dst.begin, dst.end) == (0, 200)
    assert same_events(whole(dst), tuple(None if a is None else np.concatenate([a, b[5100:5200]]) for a, b in zip(held, (x, y, t, None))))
    # an empty destination takes the source's form; a selection that keeps nothing leaves it empty and formless
    fresh = hip.EventStore(W, H, 100)
    assert fresh.select(src_pol, 0, 100, keep=np.zeros(100, np.uint8)) == 0 and not fresh.has_polarity and fresh.end == 0
    assert fresh.select(src_nopol, 0, 50) == 50 and not fresh.has_polarity
    assert status_of(hip, fresh.select, src_pol, 50, 10) == state and fresh.end == 50
