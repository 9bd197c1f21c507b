"""GPU: motion-compensated voxel grids of a reconstruction (cmx_backend_recon_voxel_* / BackendEvaluator.reconstruct_voxel_*):
the polarity-signed, time-binned event volume voted on the device, against the numpy reference of tests/recon_voxel_cases.py.

Bounds.  Default mode: every counter exactly -- tests/test_recon_voxel_cpu.py has checked that no voting event of any set lies
within 1e-9 px of a cell boundary -- and max |gpu - ref| / max(plane of ABSOLUTE votes) < RTOL of tests/util.py: the bound every
fp32-atomic plane of this suite is held to against its numpy reference, on the scale an fp32 sum's rounding follows, the
magnitude of what was added and not what remains after ON and OFF cancel.  Deterministic mode: a cell is a sum of integers, so run
to run, ingest path to ingest path, slice to slice, cut to cut and grid set to grid set it is compared bit for bit."""
import ctypes as C

import numpy as np
import pytest

import recon_cases as rc
import recon_pol_cases as pc
import recon_view_cases as vc
import recon_voxel_cases as xc
from cmax_slam_amd import _lib
from util import RTOL

pytestmark = pytest.mark.gpu
W, H = rc.SENSOR[:2]


def make(hip, case, deterministic=False):
    c, w = rc.CASES[case], rc.window(case)[0]
    be = hip.BackendEvaluator(W, H, w.lut, c["Wp"], c["Hp"])
    if deterministic:
        be.set_deterministic(True)
    return be


def begin(be, case):
    c, w = rc.CASES[case], rc.window(case)[0]
    be.reconstruct_begin(c["order"], w.knots_true, w.start_ns, w.dt_ns, c["batch"], c["rate"])


def store_of(hip, case, with_pol=True):
    _, x, y, t = rc.window(case)
    store = hip.EventStore(W, H, max(len(x), 1))
    if len(x):
        store.push(x, y, t, polarity=pc.polarity(case) if with_pol else None)
    return store


def status_of(hip, fn, *a, **k):
    with pytest.raises(hip.CmaxHipError) as e:
        fn(*a, **k)
    return e.value.status


def same(a, b):
    """two results of reconstruct_voxel_get(with_counts=True), bit for bit"""
    return a[0].shape == b[0].shape and a[0].tobytes() == b[0].tobytes() and np.array_equal(a[1], b[1])


def got(be):
    return be.reconstruct_voxel_get(with_counts=True)


def voted(hip, oracle, name, deterministic=True, only=None):
    """reconstruct_voxel_get(with_counts=True) after one voxel_add_from of the set (or of its grids `only`) over the whole stream"""
    case, Wv, Hv, n_bins, signed, grids = xc.voxel_set(oracle, name)
    be, store = make(hip, case, deterministic), store_of(hip, case)
    begin(be, case)
    be.reconstruct_voxel_begin(grids if only is None else [grids[k] for k in only], Wv, Hv, n_bins, signed)
    be.reconstruct_voxel_add_from(store, 0, rc.CASES[case]["N"])
    out = got(be)
    be.reconstruct_voxel_end()
    be.reconstruct_end()
    store.close()
    return out


def against_reference(oracle, name, out):
    planes, absp, counts, _ = xc.reference(oracle, name)
    assert out[0].shape == planes.shape and out[0].dtype == np.float32
    r = xc.rel_vox(out[0], planes, absp)
    print("%s: %s volume, %.2e of the largest |vote| sum against the reference; votes %s (reference %s)" %
          (name, planes.shape, r, out[1].tolist(), counts.tolist()))
    assert np.array_equal(out[1], counts)
    if not absp.any():
        assert not out[0].any()
    else:
        assert r < RTOL


# ---------------------------------------------------------------- 1. default mode against the reference, every set
@pytest.mark.parametrize("name", list(xc.SETS))
def test_default_mode_against_the_numpy_reference(hip, oracle, name):
    against_reference(oracle, name, voted(hip, oracle, name, deterministic=False))


@pytest.mark.parametrize("name", ["A5", "B2", "n65"])
def test_default_mode_through_the_host_paths(hip, oracle, name):
    """the packed time stream of add / add_aos, several slices"""
    case, Wv, Hv, n_bins, signed, grids = xc.voxel_set(oracle, name)
    _, x, y, t = rc.window(case)
    pol = pc.polarity(case)
    be = make(hip, case)
    begin(be, case)
    be.reconstruct_voxel_begin(grids, Wv, Hv, n_bins, signed)
    L = _lib.lib()
    try:
        assert L.cmx_diag_set(_lib.DIAG_RECON_SLICE_EVENTS, 4096) == 0
        be.reconstruct_voxel_add(x, y, t, pol)
        against_reference(oracle, name, got(be))
        be.reconstruct_voxel_reset()
        be.reconstruct_voxel_add_aos(_lib.dvs_events(x, y, t, pol))
        against_reference(oracle, name, got(be))
    finally:
        assert L.cmx_diag_set(_lib.DIAG_RECON_SLICE_EVENTS, 0) == 0
    be.reconstruct_end()


# ---------------------------------------------------------------- 2. deterministic mode, bitwise
@pytest.mark.parametrize("name", ["A5", "B2", "batch5000", "overlap10"])
def test_deterministic_mode_is_bitwise(hip, oracle, name):
    case, Wv, Hv, n_bins, signed, grids = xc.voxel_set(oracle, name)
    c = rc.CASES[case]
    _, x, y, t = rc.window(case)
    pol = pc.polarity(case)
    n, B = c["N"], c["batch"]
    want = voted(hip, oracle, name)
    against_reference(oracle, name, want)
    assert same(voted(hip, oracle, name), want)  # run to run
    be, store = make(hip, case, True), store_of(hip, case)
    begin(be, case)
    be.reconstruct_voxel_begin(grids, Wv, Hv, n_bins, signed)
    records = _lib.dvs_events(x, y, t, pol)
    paths = ((be.reconstruct_voxel_add_from, (store, 0, n)), (be.reconstruct_voxel_add, (x, y, t, pol)),
             (be.reconstruct_voxel_add_aos, (records,)))
    L = _lib.lib()
    try:
        for n_slice in (0, 2 * B, 4096):  # the default (one slice); two batches per slice; a few slices
            assert L.cmx_diag_set(_lib.DIAG_RECON_SLICE_EVENTS, n_slice) == 0
            for fn, args in paths:
                be.reconstruct_voxel_reset()
                fn(*args)
                assert same(got(be), want), (n_slice, fn.__name__)
    finally:
        assert L.cmx_diag_set(_lib.DIAG_RECON_SLICE_EVENTS, 0) == 0
    # add(A); add(B) cut at a batch multiple against add(A || B)
    cut = max(B, (n // (3 * B)) * B)
    assert 0 < cut < n - 1
    be.reconstruct_voxel_reset()
    be.reconstruct_voxel_add_from(store, 0, cut)
    be.reconstruct_voxel_add_from(store, cut, n - cut)
    assert same(got(be), want)
    be.reconstruct_voxel_reset()
    be.reconstruct_voxel_add(x[:cut], y[:cut], t[:cut], pol[:cut])
    be.reconstruct_voxel_add_aos(records[cut:])
    assert same(got(be), want)
    # a sub-range of the set through get
    part = be.reconstruct_voxel_get(1, len(grids) - 1, with_counts=True)
    assert part[0].tobytes() == want[0][1:].tobytes() and np.array_equal(part[1], want[1][1:])
    be.reconstruct_end()
    store.close()
    # with and without the other grids of the set present, and in another order
    for j in sorted({0, len(grids) // 2, len(grids) - 1}):
        alone = voted(hip, oracle, name, only=[j])
        assert alone[1][0] > 0
        assert alone[0][0].tobytes() == want[0][j].tobytes() and alone[1][0] == want[1][j], j
    back = voted(hip, oracle, name, only=list(range(len(grids)))[::-1])
    assert back[0][::-1].tobytes() == want[0].tobytes() and np.array_equal(back[1][::-1], want[1])


# ---------------------------------------------------------------- 3. out= a torch tensor on the device
def test_out_tensor_on_the_device(hip, oracle):
    torch = pytest.importorskip("torch")
    name = "A5"
    case, Wv, Hv, n_bins, signed, grids = xc.voxel_set(oracle, name)
    be, store = make(hip, case, True), store_of(hip, case)
    begin(be, case)
    be.reconstruct_voxel_begin(grids, Wv, Hv, n_bins, signed)
    be.reconstruct_voxel_add_from(store, 0, rc.CASES[case]["N"])
    host, counts = got(be)
    dev = torch.device("cuda", 0)
    full = torch.full((len(grids), n_bins, Hv, Wv), 7.0, dtype=torch.float32, device=dev)
    whole = torch.full((len(grids), n_bins, Hv, Wv), 7.0, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()  # (the fills run on torch's stream, the calls below on the context's)
    ret, cnt = be.reconstruct_voxel_get(out=full, with_counts=True)
    assert ret is full and np.array_equal(cnt, counts)
    assert full.cpu().numpy().tobytes() == host.tobytes()
    # a sub-range fills only its part
    assert be.reconstruct_voxel_get(1, 1, out=whole[1:2]) is not None
    back = whole.cpu().numpy()
    assert back[1].tobytes() == host[1].tobytes() and (back[0] == 7.0).all() and (back[2] == 7.0).all()
    assert status_of(hip, be.reconstruct_voxel_get, 2, 2, out=whole) == _lib.ERR_INVALID_ARG
    assert (whole.cpu().numpy()[0] == 7.0).all()
    # default mode: the same planes the host get reads
    be.reconstruct_end()
    be.set_deterministic(False)
    begin(be, case)
    be.reconstruct_voxel_begin(grids, Wv, Hv, n_bins, signed)
    be.reconstruct_voxel_add_from(store, 0, rc.CASES[case]["N"])
    be.reconstruct_voxel_get(out=full)
    assert full.cpu().numpy().tobytes() == be.reconstruct_voxel_get().tobytes()
    be.reconstruct_end()
    store.close()


# ---------------------------------------------------------------- 4. coexistence and life cycle
def test_a_view_set_and_a_voxel_set_side_by_side(hip, oracle):
    name = "A5"
    case, Wv, Hv, n_bins, signed, grids = xc.voxel_set(oracle, name)
    _, vWv, vHv, views = vc.view_set(oracle, "frames8")
    c, (w, x, y, t) = rc.CASES[case], rc.window(case)
    n = c["N"]
    want = voted(hip, oracle, name)
    be, store = make(hip, case, True), store_of(hip, case)
    begin(be, case)
    be.reconstruct_view_begin(views, vWv, vHv)
    be.reconstruct_view_add_from(store, 0, n)
    views_alone = be.reconstruct_view_get(with_counts=True)
    be.reconstruct_view_reset()
    be.reconstruct_add_from(store, 0, n)
    plane = be.reconstruct_get(with_counts=True)

    def untouched():
        now = be.reconstruct_get(with_counts=True)
        assert now[0].tobytes() == plane[0].tobytes() and now[1:] == plane[1:]

    be.reconstruct_voxel_begin(grids, Wv, Hv, n_bins, signed)
    zero = got(be)
    assert zero[0].shape == (len(grids), n_bins, Hv, Wv) and not zero[0].any() and not zero[1].any()
    # each voted in turn, in halves
    half = (n // (2 * c["batch"])) * c["batch"]
    be.reconstruct_voxel_add_from(store, 0, half)
    be.reconstruct_view_add_from(store, 0, half)
    be.reconstruct_voxel_add_from(store, half, n - half)
    be.reconstruct_view_add_from(store, half, n - half)
    assert same(got(be), want)
    both = be.reconstruct_view_get(with_counts=True)
    assert both[0].tobytes() == views_alone[0].tobytes() and np.array_equal(both[1], views_alone[1])
    untouched()
    # view_reset and view_end leave the voxel set alone, voxel_reset clears it and keeps the grids
    be.reconstruct_view_reset()
    assert same(got(be), want)
    be.reconstruct_voxel_reset()
    cleared = got(be)
    assert cleared[0].shape == want[0].shape and not cleared[0].any() and not cleared[1].any()
    assert not be.reconstruct_view_get().any()
    be.reconstruct_voxel_add_from(store, 0, n)
    assert same(got(be), want)
    be.reconstruct_voxel_add_from(store, 0, n)  # accumulation goes on after a get
    assert np.array_equal(got(be)[1], 2 * want[1])
    be.reconstruct_view_end()
    # restart clears and keeps the grids
    be.reconstruct_restart(w.knots_true)
    assert not got(be)[0].any() and not got(be)[1].any()
    be.reconstruct_voxel_add_from(store, 0, n)
    assert same(got(be), want)
    # a second voxel_begin starts over
    be.reconstruct_voxel_begin(grids[:2], Wv, Hv, n_bins, signed)
    assert got(be)[0].shape == (2, n_bins, Hv, Wv) and not got(be)[0].any()
    be.reconstruct_voxel_add_from(store, 0, n)
    assert got(be)[0].tobytes() == want[0][:2].tobytes()
    # voxel_end, and recon_begin, free the set
    be.reconstruct_voxel_end()
    assert status_of(hip, be.reconstruct_voxel_add_from, store, 0, n) == _lib.ERR_STATE
    assert be.reconstruct_voxel_end() is None  # voxel_end without a set is not an error
    be.reconstruct_voxel_begin(grids, Wv, Hv, n_bins, signed)
    begin(be, case)
    assert status_of(hip, be.reconstruct_voxel_add_from, store, 0, n) == _lib.ERR_STATE
    assert status_of(hip, be.reconstruct_voxel_get) == _lib.ERR_STATE
    be.reconstruct_end()
    store.close()


def test_an_unsigned_set_reads_no_polarity(hip, oracle):
    name = "one_bin"
    case, Wv, Hv, n_bins, signed, grids = xc.voxel_set(oracle, name)
    assert not signed
    _, x, y, t = rc.window(case)
    n = rc.CASES[case]["N"]
    want = voted(hip, oracle, name)
    be, bare = make(hip, case, True), store_of(hip, case, with_pol=False)
    begin(be, case)
    be.reconstruct_voxel_begin(grids, Wv, Hv, n_bins, signed=False)
    plain = _lib.dvs_events(x, y, t)
    for fn, args in ((be.reconstruct_voxel_add, (x, y, t)), (be.reconstruct_voxel_add, (x, y, t, np.zeros(n, np.uint8))),
                     (be.reconstruct_voxel_add_aos, (plain,)), (be.reconstruct_voxel_add_from, (bare, 0, n))):
        be.reconstruct_voxel_reset()
        fn(*args)
        assert same(got(be), want), fn.__name__
    be.reconstruct_end()
    bare.close()


# ---------------------------------------------------------------- 5. status codes
def test_status_codes(hip, oracle):
    name = "A5"
    case, Wv, Hv, n_bins, signed, grids = xc.voxel_set(oracle, name)
    c, (w, x, y, t) = rc.CASES[case], rc.window(case)
    pol = pc.polarity(case)
    n = c["N"]
    L = _lib.lib()
    be, store, bare = make(hip, case, True), store_of(hip, case), store_of(hip, case, with_pol=False)
    # before recon_begin, and on a group handle
    for fn, args in ((be.reconstruct_voxel_begin, (grids, Wv, Hv, n_bins)), (be.reconstruct_voxel_add, (x, y, t, pol)),
                     (be.reconstruct_voxel_add_aos, (_lib.dvs_events(x, y, t, pol),)), (be.reconstruct_voxel_add_from, (store, 0, n)),
                     (be.reconstruct_voxel_get, ()), (be.reconstruct_voxel_reset, ()), (be.reconstruct_voxel_end, ())):
        assert status_of(hip, fn, *args) == _lib.ERR_STATE, fn.__name__
    assert L.cmx_backend_recon_voxel_get_device(be._ctx, 0, 1, None) == _lib.ERR_STATE
    grp = hip.BackendEvaluator(W, H, w.lut, c["Wp"], c["Hp"], devices=[0, 0], transport=_lib.GROUP_DIRECT)
    assert status_of(hip, grp.reconstruct_voxel_begin, grids, Wv, Hv, n_bins) == _lib.ERR_STATE
    assert status_of(hip, grp.reconstruct_voxel_add, x, y, t, pol) == _lib.ERR_STATE
    assert status_of(hip, grp.reconstruct_voxel_get) == _lib.ERR_STATE
    grp.close()
    begin(be, case)
    # before voxel_begin
    for fn, args in ((be.reconstruct_voxel_add, (x, y, t, pol)), (be.reconstruct_voxel_add_aos, (_lib.dvs_events(x, y, t, pol),)),
                     (be.reconstruct_voxel_add_from, (store, 0, n)), (be.reconstruct_voxel_get, ()), (be.reconstruct_voxel_reset, ())):
        assert status_of(hip, fn, *args) == _lib.ERR_STATE, fn.__name__
    assert L.cmx_backend_recon_voxel_get_device(be._ctx, 0, 1, None) == _lib.ERR_STATE
    # every argument rule of begin
    q, fx, fy, cx, cy, lo, hi = grids[0]
    nan, inf = float("nan"), float("inf")
    g0 = grids[0]
    bad_sets = [([g0], 3, 64, 2), ([g0], 64, 3, 2), ([g0], 8193, 64, 2), ([g0], 64, 8193, 2), ([], 64, 64, 2),
                ([g0], Wv, Hv, 0), ([g0], Wv, Hv, 65), ([g0], Wv, Hv, -1),
                ([g0] * 4097, 4, 4, 1), ([g0] * 65, 4, 4, 64), ([g0] * 5, 8192, 8192, 1), ([g0] * 3, 4096, 4096, 6),  # cells > 2^28
                ([(np.zeros(4), fx, fy, cx, cy, lo, hi)], Wv, Hv, 2), ([(np.array([0, nan, 0, 1.0]), fx, fy, cx, cy, lo, hi)], Wv, Hv, 2),
                ([(q, 0.0, fy, cx, cy, lo, hi)], Wv, Hv, 2), ([(q, fx, inf, cx, cy, lo, hi)], Wv, Hv, 2),
                ([(q, fx, fy, nan, cy, lo, hi)], Wv, Hv, 2), ([(q, fx, fy, cx, inf, lo, hi)], Wv, Hv, 2),
                ([(q, fx, fy, cx, cy, hi, hi)], Wv, Hv, 2), ([(q, fx, fy, cx, cy, hi, lo)], Wv, Hv, 2),
                ([(q, fx, fy, cx, cy, lo, lo + 2 ** 53 + 1)], Wv, Hv, 2), ([(q, fx, fy, cx, cy) + vc.ALL_TIME], Wv, Hv, 2),
                ([(q, fx, fy, cx, cy, -2 ** 63, 2 ** 63 - 1)], Wv, Hv, 1),  # the difference does not fit an int64
                ([g0, (q, fx, fy, cx, cy) + vc.ALL_TIME], Wv, Hv, 2)]
    for gs, wv, hv, nb in bad_sets:
        assert status_of(hip, be.reconstruct_voxel_begin, gs, wv, hv, nb) == _lib.ERR_INVALID_ARG, (len(gs), wv, hv, nb)
    assert status_of(hip, be.reconstruct_voxel_get) == _lib.ERR_STATE  # a refused begin makes no set
    assert L.cmx_backend_recon_voxel_begin(be._ctx, Wv, Hv, 2, 1, 1, None) == _lib.ERR_INVALID_ARG
    be.reconstruct_voxel_begin([(q, fx, fy, cx, cy, lo, lo + 2 ** 53)] * 64, 4, 4, 64)  # the limits themselves
    be.reconstruct_voxel_begin([((0, 0, 0, 2.0), fx, fy, cx, cy, lo, hi)], 4, 8192, 1)  # ... and any length of quaternion
    be.reconstruct_voxel_begin(grids, Wv, Hv, n_bins, signed)
    be.reconstruct_voxel_add_from(store, 0, n)
    snap = got(be)
    assert (snap[1] > 0).all()

    def untouched():
        assert same(got(be), snap)

    # a signed set needs polarity
    assert status_of(hip, be.reconstruct_voxel_add, x, y, t) == _lib.ERR_INVALID_ARG
    assert status_of(hip, be.reconstruct_voxel_add_from, bare, 0, n) == _lib.ERR_STATE
    records = _lib.dvs_events(x, y, t, pol)
    lay = _lib.aos_layout_of(records)
    assert L.cmx_backend_recon_voxel_add_aos(be._ctx, n, records.ctypes.data, C.byref(lay), 16) == _lib.ERR_INVALID_ARG
    untouched()
    try:
        assert L.cmx_diag_set(_lib.DIAG_RECON_SLICE_EVENTS, 4096) == 0   # several slices: the bad event sits in the last one
        bad_x = x.copy()
        bad_x[-2] = W
        assert status_of(hip, be.reconstruct_voxel_add, bad_x, y, t, pol) == _lib.ERR_EVENT_RANGE
        bad_y = y.copy()
        bad_y[-2] = H
        assert status_of(hip, be.reconstruct_voxel_add_aos, _lib.dvs_events(x, bad_y, t, pol)) == _lib.ERR_EVENT_RANGE
        untouched()
        back = t.copy()
        back[n - 107] = t[n - 8] + 1000  # the first event of the last batch later than its last one
        assert (n - 107) % c["batch"] == 0
        assert status_of(hip, be.reconstruct_voxel_add, x, y, back, pol) == _lib.ERR_TIME_ORDER
        st = hip.EventStore(W, H, n)
        st.push(x, y, back, polarity=pol)
        assert status_of(hip, be.reconstruct_voxel_add_from, st, 0, n) == _lib.ERR_TIME_ORDER
        st.close()
        untouched()
        tail = t.copy()
        tail[-150:] += 10_000_000_000  # batch times outside the spline: the last two batches alone
        assert status_of(hip, be.reconstruct_voxel_add, x, y, tail, pol) == _lib.ERR_SPLINE_RANGE
        assert status_of(hip, be.reconstruct_voxel_add_aos, _lib.dvs_events(x, y, tail, pol)) == _lib.ERR_SPLINE_RANGE
        st = hip.EventStore(W, H, n)
        st.push(x, y, tail, polarity=pol)
        assert status_of(hip, be.reconstruct_voxel_add_from, st, 0, n) == _lib.ERR_SPLINE_RANGE
        st.close()
        untouched()
    finally:
        assert L.cmx_diag_set(_lib.DIAG_RECON_SLICE_EVENTS, 0) == 0
    assert status_of(hip, be.reconstruct_voxel_add_from, store, 0, n + 1) == _lib.ERR_INVALID_ARG
    # get arguments
    for first, count in ((-1, 1), (0, 4), (3, 1), (4, 0), (0, -1)):
        assert status_of(hip, be.reconstruct_voxel_get, first, count) == _lib.ERR_INVALID_ARG, (first, count)
    assert be.reconstruct_voxel_get(3, 0).shape == (0, n_bins, Hv, Wv)
    assert L.cmx_backend_recon_voxel_get_device(be._ctx, 0, 1, None) == _lib.ERR_INVALID_ARG
    counts_only = np.zeros(3, np.int64)
    assert L.cmx_backend_recon_voxel_get(be._ctx, 0, 3, None, counts_only.ctypes.data_as(_lib.c_i64p)) == _lib.OK
    assert np.array_equal(counts_only, snap[1])
    untouched()
    be.reconstruct_end()
    store.close()
    bare.close()


# ---------------------------------------------------------------- helpers of the public interface
def test_voxel_grids_helper(hip, oracle):
    from cmax_slam_amd import trajectory
    case = "A"
    c, (w, x, y, t) = rc.CASES[case], rc.window(case)
    pol = pc.polarity(case)
    grids = trajectory.voxel_grids(c["order"], w.knots_true, w.start_ns, w.dt_ns, 1_000_000_000, vc.scaled_intrinsics(96, 64))
    as_tuples = [(np.array(g.quat_xyzw), g.fx, g.fy, g.cx, g.cy, g.t_lo_ns, g.t_hi_ns) for g in grids]
    planes, absp, counts, _ = xc.reference_of(oracle, case, as_tuples, 96, 64, 3, True, x, y, t, pol)
    be = make(hip, case, True)
    begin(be, case)
    be.reconstruct_voxel_begin(grids, 96, 64, 3)
    be.reconstruct_voxel_add(x, y, t, pol)
    out = got(be)
    be.reconstruct_end()
    assert len(grids) >= 4 and np.array_equal(out[1], counts) and (counts > 1000).all()
    assert xc.rel_vox(out[0], planes, absp) < RTOL


# ---------------------------------------------------------------- example
def test_example_writes_one_npy_of_voxel_grids(hip, tmp_path):
    import os
    import sys
    from cmax_slam_amd import synth
    ex = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples")
    if ex not in sys.path:
        sys.path.insert(0, ex)
    import rotation_pipeline as rp
    stream = synth.event_stream(2e6, 0.5, 240, 180, 200.0, 200.0, 119.5, 89.5, omega_mean=(0.2, 1.8, 0.3), omega_amp=(1.0, 0.8, 1.0), seed=77)
    path = str(tmp_path / "volumes.npy")
    res = rp.run_pipeline(stream, rp.Params(), voxels=path, voxel_ms=50.0, voxel_bins=4)
    volumes, counts = res["voxels"]
    on_disk = np.load(path)
    print("example: %s volumes, %s events each" % (volumes.shape, counts.tolist()))
    assert on_disk.shape == volumes.shape == (len(counts), 4, 180, 240) and len(counts) >= 5 and on_disk.dtype == np.float32
    assert on_disk.tobytes() == volumes.tobytes()
    assert (counts > 0).all()  # no grid inside the recording is empty
    assert (volumes > 0).any(axis=(2, 3)).all() and (volumes < 0).any(axis=(2, 3)).all()  # every bin holds ON and OFF votes
    text = open(os.path.join(ex, "rotation_pipeline.py")).read()
    assert "--voxels" in text and "--voxel-ms" in text and "--voxel-bins" in text
