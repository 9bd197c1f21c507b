"""GPU: motion-compensated time surfaces of a reconstruction (cmx_backend_recon_surface_* / BackendEvaluator.reconstruct_surface_*):
the latest event per pixel and polarity, voted on the device as one 64-bit integer max, against the numpy reference of
tests/recon_surface_cases.py.

Bounds.  A cell is a maximum of integers: there is no rounding, so counters AND cells are compared exactly, in default and in
deterministic mode alike -- up to two cells per voting event within recon_warp_cases.NEAR_INTEGER of a half-pixel boundary, of which
tests/test_recon_surface_cpu.py has found none in any set, so the cells are equal everywhere.  Run to run, ingest path to ingest
path, slice to slice, cut to cut IN EITHER ORDER, set to set and mode to mode the cells are compared bit for bit.  The decayed
surfaces: 0.0f and 1.0f exactly where the header says so, and one fp32 ulp elsewhere -- both sides take an fp64 exp good to an ulp
or two of fp64 and round once to fp32, so they can only part where that fp64 difference straddles an fp32 rounding boundary."""
import ctypes as C

import numpy as np
import pytest

import recon_cases as rc
import recon_pol_cases as pc
import recon_surface_cases as sc
import recon_view_cases as vc
import recon_voxel_cases as xc
from cmax_slam_amd import _lib

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
    """two results of reconstruct_surface_get(with_counts=True), bit for bit"""
    return a[0].shape == b[0].shape and a[0].tobytes() == b[0].tobytes() and np.array_equal(a[1], b[1])


def got(be):
    return be.reconstruct_surface_get(with_counts=True)


def voted(hip, oracle, name, deterministic=False, only=None, by_polarity=None):
    """reconstruct_surface_get(with_counts=True) after one surface_add_from of the set (or of its surfaces `only`) over the stream"""
    case, Wv, Hv, by_pol, surfaces = sc.surface_set(oracle, name)
    be, store = make(hip, case, deterministic), store_of(hip, case)
    begin(be, case)
    be.reconstruct_surface_begin(surfaces if only is None else [surfaces[k] for k in only], Wv, Hv,
                                 by_pol if by_polarity is None else by_polarity)
    be.reconstruct_surface_add_from(store, 0, rc.CASES[case]["N"])
    out = got(be)
    be.reconstruct_surface_end()
    be.reconstruct_end()
    store.close()
    return out


def against_reference(oracle, name, out):
    cells, counts, near, _, _ = sc.reference(oracle, name)
    assert out[0].shape == cells.shape and out[0].dtype == np.int64
    differ = int(np.count_nonzero(out[0] != cells))
    print("%s: %s cells, %d differ from the reference (%d near-boundary events); votes %s (reference %s)" %
          (name, cells.shape, differ, near, out[1].tolist(), counts.tolist()))
    assert np.array_equal(out[1], counts)
    assert differ <= 2 * near
    if near == 0:
        assert np.array_equal(out[0], cells)


# ---------------------------------------------------------------- 1. every set against the reference
@pytest.mark.parametrize("name", sc.SETS)
def test_every_set_against_the_numpy_reference(hip, oracle, name):
    against_reference(oracle, name, voted(hip, oracle, name))


@pytest.mark.parametrize("name", ["A5", "B2", "n65"])
def test_against_the_reference_through_the_host_paths(hip, oracle, name):
    """the packed time stream of add / add_aos, several slices"""
    case, Wv, Hv, by_pol, surfaces = sc.surface_set(oracle, name)
    _, x, y, t = rc.window(case)
    pol = pc.polarity(case)
    be = make(hip, case)
    begin(be, case)
    be.reconstruct_surface_begin(surfaces, Wv, Hv, by_pol)
    L = _lib.lib()
    try:
        assert L.cmx_diag_set(_lib.DIAG_RECON_SLICE_EVENTS, 4096) == 0
        be.reconstruct_surface_add(x, y, t, pol)
        against_reference(oracle, name, got(be))
        be.reconstruct_surface_reset()
        be.reconstruct_surface_add_aos(_lib.dvs_events(x, y, t, pol))
        against_reference(oracle, name, got(be))
    finally:
        assert L.cmx_diag_set(_lib.DIAG_RECON_SLICE_EVENTS, 0) == 0
    be.reconstruct_end()


# ---------------------------------------------------------------- 2. bitwise, in default and in deterministic mode
@pytest.mark.parametrize("name", ["A5", "B2", "batch5000", "overlap10"])
def test_bitwise_in_both_modes(hip, oracle, name):
    case, Wv, Hv, by_pol, surfaces = sc.surface_set(oracle, name)
    c = rc.CASES[case]
    _, x, y, t = rc.window(case)
    pol = pc.polarity(case)
    n, B = c["N"], c["batch"]
    records = _lib.dvs_events(x, y, t, pol)
    wants = []
    L = _lib.lib()
    for det in (False, True):
        want = voted(hip, oracle, name, det)
        against_reference(oracle, name, want)
        assert same(voted(hip, oracle, name, det), want)  # run to run
        be, store = make(hip, case, det), store_of(hip, case)
        begin(be, case)
        be.reconstruct_surface_begin(surfaces, Wv, Hv, by_pol)
        paths = ((be.reconstruct_surface_add_from, (store, 0, n)), (be.reconstruct_surface_add, (x, y, t, pol)),
                 (be.reconstruct_surface_add_aos, (records,)))
        try:
            for n_slice in (0, 2 * B, 4096):  # the default (one slice); two batches per slice; a few slices
                assert L.cmx_diag_set(_lib.DIAG_RECON_SLICE_EVENTS, n_slice) == 0
                for fn, args in paths:
                    be.reconstruct_surface_reset()
                    fn(*args)
                    assert same(got(be), want), (det, n_slice, fn.__name__)
        finally:
            assert L.cmx_diag_set(_lib.DIAG_RECON_SLICE_EVENTS, 0) == 0
        # add(A); add(B) cut at a batch multiple against add(A || B) ...
        cut = max(B, (n // (3 * B)) * B)
        assert 0 < cut < n - 1
        be.reconstruct_surface_reset()
        be.reconstruct_surface_add_from(store, 0, cut)
        be.reconstruct_surface_add_from(store, cut, n - cut)
        assert same(got(be), want)
        # ... and add(B); add(A), the later half first: a store in place of a max fails this
        be.reconstruct_surface_reset()
        be.reconstruct_surface_add_from(store, cut, n - cut)
        be.reconstruct_surface_add_from(store, 0, cut)
        assert same(got(be), want)
        be.reconstruct_surface_reset()
        be.reconstruct_surface_add_aos(records[cut:])
        be.reconstruct_surface_add(x[:cut], y[:cut], t[:cut], pol[:cut])
        assert same(got(be), want)
        # a max is idempotent: the same events again change no cell and double the counters
        be.reconstruct_surface_add_from(store, 0, n)
        again = got(be)
        assert again[0].tobytes() == want[0].tobytes() and np.array_equal(again[1], 2 * want[1])
        # a sub-range of the set through get
        part = be.reconstruct_surface_get(1, len(surfaces) - 1, with_counts=True)
        assert part[0].tobytes() == want[0][1:].tobytes() and np.array_equal(part[1], 2 * want[1][1:])
        be.reconstruct_end()
        store.close()
        # with and without the other surfaces of the set present, and in another order
        for j in sorted({0, len(surfaces) // 2, len(surfaces) - 1}):
            alone = voted(hip, oracle, name, det, only=[j])
            assert alone[1][0] > 0
            assert alone[0][0].tobytes() == want[0][j].tobytes() and alone[1][0] == want[1][j], j
        back = voted(hip, oracle, name, det, only=list(range(len(surfaces)))[::-1])
        assert back[0][::-1].tobytes() == want[0].tobytes() and np.array_equal(back[1][::-1], want[1])
        wants.append(want)
    assert same(wants[0], wants[1])  # deterministic mode against default mode: the option changes nothing here


# ---------------------------------------------------------------- 3. channels
@pytest.mark.parametrize("name", ["A5", "batch5000"])
def test_maximum_of_the_channels_is_the_merged_set(hip, oracle, name):
    case, Wv, Hv, by_pol, surfaces = sc.surface_set(oracle, name)
    assert by_pol
    split, merged = voted(hip, oracle, name), voted(hip, oracle, name, by_polarity=False)
    assert merged[0].shape == (len(surfaces), 1, Hv, Wv) and np.array_equal(split[1], merged[1])
    assert (split[0][:, 0] != sc.EMPTY).any() and (split[0][:, 1] != sc.EMPTY).any()
    assert np.maximum(split[0][:, 0], split[0][:, 1]).tobytes() == merged[0][:, 0].tobytes()


def test_a_merged_set_reads_no_polarity(hip, oracle):
    name = "one_bin"
    case, Wv, Hv, by_pol, surfaces = sc.surface_set(oracle, name)
    assert not by_pol
    _, x, y, t = rc.window(case)
    n = rc.CASES[case]["N"]
    want = voted(hip, oracle, name)
    against_reference(oracle, name, want)
    be, bare = make(hip, case), store_of(hip, case, with_pol=False)
    begin(be, case)
    be.reconstruct_surface_begin(surfaces, Wv, Hv, by_polarity=False)
    plain = _lib.dvs_events(x, y, t)
    for fn, args in ((be.reconstruct_surface_add, (x, y, t)), (be.reconstruct_surface_add, (x, y, t, np.zeros(n, np.uint8))),
                     (be.reconstruct_surface_add_aos, (plain,)), (be.reconstruct_surface_add_from, (bare, 0, n))):
        be.reconstruct_surface_reset()
        fn(*args)
        assert same(got(be), want), fn.__name__
    be.reconstruct_end()
    bare.close()


@pytest.mark.parametrize("name", ["A5", "B2", "batch5000", "overlap10", "poles"])
def test_counts_are_those_of_a_voxel_set_over_the_same_grids(hip, oracle, name):
    """the same membership rule (the event's own timestamp) and the same vote test"""
    case, Wv, Hv, n_bins, signed, grids = xc.voxel_set(oracle, name)
    be, store = make(hip, case), store_of(hip, case)
    n = rc.CASES[case]["N"]
    begin(be, case)
    be.reconstruct_voxel_begin(grids, Wv, Hv, n_bins, signed)
    be.reconstruct_surface_begin(grids, Wv, Hv, True)
    be.reconstruct_voxel_add_from(store, 0, n)
    be.reconstruct_surface_add_from(store, 0, n)
    vox = be.reconstruct_voxel_get(with_counts=True)[1]
    assert np.array_equal(got(be)[1], vox) and (vox > 0).all()
    be.reconstruct_end()
    store.close()


# ---------------------------------------------------------------- 4. decay, and the device outputs
def ulps(a, b):
    """the distance of two arrays of non-negative finite fp32 in units of the last place"""
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


def test_decay_and_device_outputs(hip, oracle):
    torch = pytest.importorskip("torch")
    name = "A5"
    case, Wv, Hv, by_pol, surfaces = sc.surface_set(oracle, name)
    be, store = make(hip, case), store_of(hip, case)
    begin(be, case)
    be.reconstruct_surface_begin(surfaces, Wv, Hv, by_pol)
    be.reconstruct_surface_add_from(store, 0, rc.CASES[case]["N"])
    cells, counts = got(be)
    against_reference(oracle, name, (cells, counts))
    S = len(surfaces)
    lo = np.array([g[5] for g in surfaces], np.int64)
    hi = np.array([g[6] for g in surfaces], np.int64)
    span = int((hi - lo).max())
    dev = torch.device("cuda", 0)
    empty = cells == sc.EMPTY
    assert empty.any() and (~empty).any()
    for tau in (span / 10.0, float(span)):  # (t_ref - T) / tau <= 10: nothing near FLT_MIN
        for t_ref in (None, (lo + hi) // 2):
            ref_t = hi if t_ref is None else t_ref
            want = sc.decay_reference(cells, ref_t, tau)
            host = be.reconstruct_surface_decay(tau, t_ref)
            assert host.shape == cells.shape and host.dtype == np.float32
            late = ~empty & (cells >= ref_t[:, None, None, None])
            assert (host[empty] == 0.0).all() and (host[late] == 1.0).all()
            assert late.any() == (t_ref is not None)  # NULL t_ref is t_hi: no event of a surface is that late
            rest = ~empty & ~late
            assert rest.any() and (want[rest] > 1e-5).all()  # normal numbers all (an event just before t_ref may round to 1.0f)
            d = ulps(host[rest], want[rest])
            print("decay tau=%.3g t_ref=%s: %d cells, %d one ulp off, max %d ulp" %
                  (tau, "t_hi" if t_ref is None else "mid", int(rest.sum()), int((d == 1).sum()), int(d.max())))
            assert d.max() <= 1
            out = torch.full(cells.shape, 7.0, dtype=torch.float32, device=dev)
            torch.cuda.synchronize()  # (the fill runs on torch's stream, the call below on the context's)
            assert be.reconstruct_surface_decay(tau, t_ref, out=out) is out
            assert out.cpu().numpy().tobytes() == host.tobytes()
    # one reference time for all, and a sub-range fills only its part
    tau = float(span)
    whole = torch.full(cells.shape, 7.0, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    be.reconstruct_surface_decay(tau, int(hi[1]), first=1, count=1, out=whole[1:2])
    back = whole.cpu().numpy()
    assert back[1].tobytes() == be.reconstruct_surface_decay(tau, None, 1, 1).tobytes()
    assert (back[0] == 7.0).all() and (back[2] == 7.0).all()
    # get(out=int64 tensor) is bitwise the host get
    full = torch.full(cells.shape, 7, dtype=torch.int64, device=dev)
    part = torch.full(cells.shape, 7, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    ret, cnt = be.reconstruct_surface_get(out=full, with_counts=True)
    assert ret is full and np.array_equal(cnt, counts) and full.cpu().numpy().tobytes() == cells.tobytes()
    be.reconstruct_surface_get(S - 1, 1, out=part[S - 1:])
    back = part.cpu().numpy()
    assert back[S - 1].tobytes() == cells[S - 1].tobytes() and (back[:S - 1] == 7).all()
    assert status_of(hip, be.reconstruct_surface_get, 2, 2, out=part) == _lib.ERR_INVALID_ARG
    assert status_of(hip, be.reconstruct_surface_decay, tau, None, 2, 2, out=whole) == _lib.ERR_INVALID_ARG
    assert (part.cpu().numpy()[0] == 7).all() and (whole.cpu().numpy()[0] == 7.0).all()
    # the decay leaves the cells as they are
    assert same(got(be), (cells, counts))
    be.reconstruct_end()
    store.close()


def test_decay_over_all_time(hip, oracle):
    """a reference time far from the cells: the difference is formed without signed overflow"""
    name = "all_time"
    case, Wv, Hv, by_pol, surfaces = sc.surface_set(oracle, name)
    be, store = make(hip, case), store_of(hip, case)
    begin(be, case)
    be.reconstruct_surface_begin(surfaces, Wv, Hv, by_pol)
    be.reconstruct_surface_add_from(store, 0, rc.CASES[case]["N"])
    cells, _ = got(be)
    reached = cells != sc.EMPTY
    # t_hi = 2^62 and tau = 2^60: (t_ref - T) / tau is about 4
    host = be.reconstruct_surface_decay(float(2 ** 60))
    want = sc.decay_reference(cells, [surfaces[0][6]], float(2 ** 60))
    assert (host[~reached] == 0.0).all() and ulps(host[reached], want[reached]).max() <= 1 and (host[reached] > 0.01).all()
    # t_ref = INT64_MAX against cells near 0 with tau = 2^62: the signed difference of t_ref and T = -1 would overflow
    top = 2 ** 63 - 1
    host = be.reconstruct_surface_decay(float(2 ** 62), top)
    want = sc.decay_reference(cells, [top], float(2 ** 62))
    assert ulps(host[reached], want[reached]).max() <= 1 and (host[reached] > 0.1).all() and (host[reached] < 0.2).all()
    be.reconstruct_end()
    store.close()


# ---------------------------------------------------------------- 5. side by side
def test_view_voxel_and_surface_sets_side_by_side(hip, oracle):
    name = "A5"
    case, Wv, Hv, by_pol, surfaces = sc.surface_set(oracle, name)
    _, _, _, n_bins, signed, grids = xc.voxel_set(oracle, name)
    _, vWv, vHv, views = vc.view_set(oracle, "frames8")
    c, (w, x, y, t) = rc.CASES[case], rc.window(case)
    pol = pc.polarity(case)
    n = c["N"]
    want = voted(hip, oracle, name)
    be, store = make(hip, case, True), store_of(hip, case)
    begin(be, case)
    be.reconstruct_add_from(store, 0, n)
    be.reconstruct_view_begin(views, vWv, vHv)
    be.reconstruct_view_add_from(store, 0, n)
    be.reconstruct_voxel_begin(grids, Wv, Hv, n_bins, signed)
    be.reconstruct_voxel_add_from(store, 0, n)

    def others():
        plane = be.reconstruct_get(with_counts=True)
        vw = be.reconstruct_view_get(with_counts=True)
        vx = be.reconstruct_voxel_get(with_counts=True)
        return (plane[0].tobytes(), plane[1:], vw[0].tobytes(), vw[1].tolist(), vx[0].tobytes(), vx[1].tolist())

    before = others()
    be.reconstruct_surface_begin(surfaces, Wv, Hv, by_pol)
    fresh = got(be)
    assert fresh[0].shape == (len(surfaces), 2, Hv, Wv) and (fresh[0] == sc.EMPTY).all() and not fresh[1].any()
    half = (n // (2 * c["batch"])) * c["batch"]
    be.reconstruct_surface_add(x[half:], y[half:], t[half:], pol[half:])
    be.reconstruct_surface_add_aos(_lib.dvs_events(x[:half], y[:half], t[:half], pol[:half]))
    assert same(got(be), want) and others() == before
    be.reconstruct_surface_reset()
    be.reconstruct_surface_add_from(store, 0, n)
    assert same(got(be), want) and others() == before
    # view_add*, voxel_add* and add* leave the surfaces untouched, and so do their resets and ends
    be.reconstruct_view_add_from(store, 0, n)
    be.reconstruct_voxel_add(x, y, t, pol)
    be.reconstruct_add_from(store, 0, n)
    assert same(got(be), want)
    be.reconstruct_view_reset()
    be.reconstruct_voxel_reset()
    be.reconstruct_view_end()
    be.reconstruct_voxel_end()
    assert same(got(be), want)
    # surface_reset empties and keeps the surfaces; so does restart
    be.reconstruct_surface_reset()
    cleared = got(be)
    assert cleared[0].shape == want[0].shape and (cleared[0] == sc.EMPTY).all() and not cleared[1].any()
    be.reconstruct_surface_add_from(store, 0, n)
    assert same(got(be), want)
    be.reconstruct_restart(w.knots_true)
    cleared = got(be)
    assert (cleared[0] == sc.EMPTY).all() and not cleared[1].any()
    be.reconstruct_surface_add_from(store, 0, n)
    assert same(got(be), want)
    # a second surface_begin starts over
    be.reconstruct_surface_begin(surfaces[:2], Wv, Hv, by_pol)
    assert got(be)[0].shape == (2, 2, Hv, Wv) and (got(be)[0] == sc.EMPTY).all()
    be.reconstruct_surface_add_from(store, 0, n)
    assert got(be)[0].tobytes() == want[0][:2].tobytes()
    # surface_end, and recon_begin, free the set
    be.reconstruct_surface_end()
    assert status_of(hip, be.reconstruct_surface_add_from, store, 0, n) == _lib.ERR_STATE
    assert be.reconstruct_surface_end() is None  # surface_end without a set is not an error
    be.reconstruct_surface_begin(surfaces, Wv, Hv, by_pol)
    begin(be, case)
    assert status_of(hip, be.reconstruct_surface_add_from, store, 0, n) == _lib.ERR_STATE
    assert status_of(hip, be.reconstruct_surface_get) == _lib.ERR_STATE
    be.reconstruct_end()
    store.close()


def test_the_surface_calls_change_nothing_else(hip, oracle):
    """with a gradient pass open, with events bound, after freeze_head and after release_head"""
    case = "window"
    c, (w, x, y, t) = rc.CASES[case], rc.window(case)
    n = c["N"]
    pol = pc.polarity(case)
    surfaces = [(np.array(w.knots_true[3]),) + vc.scaled_intrinsics(96, 64) + vc.ALL_TIME,
                (np.array(w.knots_true[6]),) + vc.scaled_intrinsics(96, 64) + (int(t[n // 3]), int(t[2 * n // 3]))]
    ref = sc.reference_of(oracle, case, surfaces, 96, 64, True, x, y, t, pol)
    assert (ref[1] >= 100).all() and ref[2] == 0
    be, store = make(hip, case, True), store_of(hip, case)

    def surface_calls():
        be.reconstruct_surface_begin(surfaces, 96, 64)
        be.reconstruct_surface_add_from(store, 0, n)
        out = got(be)
        be.reconstruct_surface_decay(1e9)
        be.reconstruct_surface_end()
        assert np.array_equal(out[1], ref[1]) and np.array_equal(out[0], ref[0])
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
    surface_calls()
    be.reconstruct_grad_add_from(store, 10_000, n - 10_000)
    grad = be.reconstruct_grad_get()  # (CMX_ERR_STATE had a surface call closed the pass or touched its counts)
    assert np.abs(grad).max() > 0 and state() == before
    other = make(hip, case, True)
    begin(other, case)
    other.reconstruct_add_from(store, 0, n)
    other.reconstruct_contrast(1.0, want_grad=True)
    other.reconstruct_grad_add_from(store, 0, 10_000)  # (the same cuts: the gradient sums are bitwise per sequence of calls)
    other.reconstruct_grad_add_from(store, 10_000, n - 10_000)
    assert other.reconstruct_grad_get().tobytes() == grad.tobytes()
    other.reconstruct_bind(store, 0, n)
    be.reconstruct_bind(store, 0, n)
    for step in ("bound", "frozen", "released"):
        for e in (be, other):
            if step == "frozen":
                e.reconstruct_freeze_head(5)
            if step == "released":
                e.reconstruct_release_head()
        ev = be.reconstruct_eval_bound(None, 1.0)
        infos = (be.reconstruct_bound_info(), be.reconstruct_frozen_info(), be.reconstruct_online_info())
        before = state()
        surface_calls()
        assert state() == before
        assert (be.reconstruct_bound_info(), be.reconstruct_frozen_info(), be.reconstruct_online_info()) == infos
        ev2, ev_o = be.reconstruct_eval_bound(None, 1.0), other.reconstruct_eval_bound(None, 1.0)
        assert ev2[0] == ev[0] == ev_o[0] and ev2[1].tobytes() == ev[1].tobytes() == ev_o[1].tobytes(), step
    other.reconstruct_end()
    be.reconstruct_end()
    store.close()


# ---------------------------------------------------------------- 6. status codes
def test_status_codes(hip, oracle):
    name = "A5"
    case, Wv, Hv, by_pol, surfaces = sc.surface_set(oracle, name)
    c, (w, x, y, t) = rc.CASES[case], rc.window(case)
    pol = pc.polarity(case)
    n = c["N"]
    L = _lib.lib()
    be, store, bare = make(hip, case), store_of(hip, case), store_of(hip, case, with_pol=False)
    records = _lib.dvs_events(x, y, t, pol)
    # before recon_begin, and on a group handle
    for fn, args in ((be.reconstruct_surface_begin, (surfaces, Wv, Hv)), (be.reconstruct_surface_add, (x, y, t, pol)),
                     (be.reconstruct_surface_add_aos, (records,)), (be.reconstruct_surface_add_from, (store, 0, n)),
                     (be.reconstruct_surface_get, ()), (be.reconstruct_surface_decay, (1e6,)), (be.reconstruct_surface_reset, ()),
                     (be.reconstruct_surface_end, ())):
        assert status_of(hip, fn, *args) == _lib.ERR_STATE, fn.__name__
    assert L.cmx_backend_recon_surface_get_device(be._ctx, 0, 1, None) == _lib.ERR_STATE
    assert L.cmx_backend_recon_surface_decay_device(be._ctx, 0, 1, None, 1e6, None) == _lib.ERR_STATE
    grp = hip.BackendEvaluator(W, H, w.lut, c["Wp"], c["Hp"], devices=[0, 0], transport=_lib.GROUP_DIRECT)
    assert status_of(hip, grp.reconstruct_surface_begin, surfaces, Wv, Hv) == _lib.ERR_STATE
    assert status_of(hip, grp.reconstruct_surface_add, x, y, t, pol) == _lib.ERR_STATE
    assert status_of(hip, grp.reconstruct_surface_get) == _lib.ERR_STATE
    assert status_of(hip, grp.reconstruct_surface_decay, 1e6) == _lib.ERR_STATE
    assert status_of(hip, grp.reconstruct_surface_end) == _lib.ERR_STATE
    grp.close()
    begin(be, case)
    # before surface_begin
    for fn, args in ((be.reconstruct_surface_add, (x, y, t, pol)), (be.reconstruct_surface_add_aos, (records,)),
                     (be.reconstruct_surface_add_from, (store, 0, n)), (be.reconstruct_surface_get, ()),
                     (be.reconstruct_surface_decay, (1e6,)), (be.reconstruct_surface_reset, ())):
        assert status_of(hip, fn, *args) == _lib.ERR_STATE, fn.__name__
    assert L.cmx_backend_recon_surface_get_device(be._ctx, 0, 1, None) == _lib.ERR_STATE
    assert L.cmx_backend_recon_surface_decay_device(be._ctx, 0, 1, None, 1e6, None) == _lib.ERR_STATE
    assert be.reconstruct_surface_end() is None
    # every argument rule of begin
    q, fx, fy, cx, cy, lo, hi = surfaces[0]
    nan, inf = float("nan"), float("inf")
    g0 = surfaces[0]
    bad_sets = [([g0], 3, 64, True), ([g0], 64, 3, True), ([g0], 8193, 64, True), ([g0], 64, 8193, True), ([], 64, 64, True),
                ([g0] * 4097, 4, 4, False),
                ([g0] * 5, 8192, 8192, False), ([g0] * 3, 8192, 8192, True), ([g0] * 4096, 256, 257, False),  # cells > 2^28
                ([g0] * 2049, 256, 256, True),
                ([(np.zeros(4), fx, fy, cx, cy, lo, hi)], Wv, Hv, True), ([(np.array([0, nan, 0, 1.0]), fx, fy, cx, cy, lo, hi)], Wv, Hv, True),
                ([(q, 0.0, fy, cx, cy, lo, hi)], Wv, Hv, True), ([(q, fx, inf, cx, cy, lo, hi)], Wv, Hv, True),
                ([(q, fx, fy, nan, cy, lo, hi)], Wv, Hv, True), ([(q, fx, fy, cx, inf, lo, hi)], Wv, Hv, True),
                ([(q, fx, fy, cx, cy, hi, hi)], Wv, Hv, True), ([(q, fx, fy, cx, cy, hi, lo)], Wv, Hv, True),
                ([(q, fx, fy, cx, cy, -2 ** 63, hi)], Wv, Hv, True),  # the empty marker could be a vote
                ([g0, (q, fx, fy, cx, cy, -2 ** 63, 2 ** 63 - 1)], Wv, Hv, False)]
    for gs, wv, hv, bp in bad_sets:
        assert status_of(hip, be.reconstruct_surface_begin, gs, wv, hv, bp) == _lib.ERR_INVALID_ARG, (len(gs), wv, hv, bp)
    assert status_of(hip, be.reconstruct_surface_get) == _lib.ERR_STATE  # a refused begin makes no set
    assert L.cmx_backend_recon_surface_begin(be._ctx, Wv, Hv, 1, 1, None) == _lib.ERR_INVALID_ARG
    be.reconstruct_surface_begin([g0] * 4096, 4, 4, False)  # the limits themselves
    be.reconstruct_surface_begin([g0] * 2048, 256, 256, True)  # ... 2^28 cells exactly
    be.reconstruct_surface_begin([((0, 0, 0, 2.0), fx, fy, cx, cy, -2 ** 63 + 1, 2 ** 63 - 1)], 4, 8192, True)  # ... any range but the marker
    be.reconstruct_surface_begin([(q, fx, fy, cx, cy) + vc.ALL_TIME], Wv, Hv, True)  # all time is accepted
    be.reconstruct_surface_begin(surfaces, Wv, Hv, by_pol)
    be.reconstruct_surface_add_from(store, 0, n)
    snap = got(be)
    assert (snap[1] > 0).all()

    def untouched():
        assert same(got(be), snap)

    # a by-polarity set needs polarity
    assert status_of(hip, be.reconstruct_surface_add, x, y, t) == _lib.ERR_INVALID_ARG
    assert status_of(hip, be.reconstruct_surface_add_from, bare, 0, n) == _lib.ERR_STATE
    lay = _lib.aos_layout_of(records)
    assert L.cmx_backend_recon_surface_add_aos(be._ctx, n, records.ctypes.data, C.byref(lay), 16) == _lib.ERR_INVALID_ARG
    untouched()
    try:
        assert L.cmx_diag_set(_lib.DIAG_RECON_SLICE_EVENTS, 4096) == 0   # several slices: the bad event sits in the last one
        bad_x = x.copy()
        bad_x[-2] = W
        assert status_of(hip, be.reconstruct_surface_add, bad_x, y, t, pol) == _lib.ERR_EVENT_RANGE
        bad_y = y.copy()
        bad_y[-2] = H
        assert status_of(hip, be.reconstruct_surface_add_aos, _lib.dvs_events(x, bad_y, t, pol)) == _lib.ERR_EVENT_RANGE
        untouched()
        back = t.copy()
        back[n - 107] = t[n - 8] + 1000  # the first event of the last batch later than its last one
        assert (n - 107) % c["batch"] == 0
        assert status_of(hip, be.reconstruct_surface_add, x, y, back, pol) == _lib.ERR_TIME_ORDER
        st = hip.EventStore(W, H, n)
        st.push(x, y, back, polarity=pol)
        assert status_of(hip, be.reconstruct_surface_add_from, st, 0, n) == _lib.ERR_TIME_ORDER
        st.close()
        untouched()
        tail = t.copy()
        tail[-150:] += 10_000_000_000  # batch times outside the spline: the last two batches alone
        assert status_of(hip, be.reconstruct_surface_add, x, y, tail, pol) == _lib.ERR_SPLINE_RANGE
        assert status_of(hip, be.reconstruct_surface_add_aos, _lib.dvs_events(x, y, tail, pol)) == _lib.ERR_SPLINE_RANGE
        st = hip.EventStore(W, H, n)
        st.push(x, y, tail, polarity=pol)
        assert status_of(hip, be.reconstruct_surface_add_from, st, 0, n) == _lib.ERR_SPLINE_RANGE
        st.close()
        untouched()
    finally:
        assert L.cmx_diag_set(_lib.DIAG_RECON_SLICE_EVENTS, 0) == 0
    assert status_of(hip, be.reconstruct_surface_add_from, store, 0, n + 1) == _lib.ERR_INVALID_ARG
    # ranges outside the set, for get and for decay
    for first, count in ((-1, 1), (0, 4), (3, 1), (4, 0), (0, -1)):
        assert status_of(hip, be.reconstruct_surface_get, first, count) == _lib.ERR_INVALID_ARG, (first, count)
        assert status_of(hip, be.reconstruct_surface_decay, 1e6, None, first, count) == _lib.ERR_INVALID_ARG, (first, count)
        assert L.cmx_backend_recon_surface_decay_device(be._ctx, first, count, None, 1e6, None) == _lib.ERR_INVALID_ARG
    assert be.reconstruct_surface_get(3, 0).shape == (0, 2, Hv, Wv) and be.reconstruct_surface_decay(1e6, None, 3, 0).shape == (0, 2, Hv, Wv)
    assert L.cmx_backend_recon_surface_get_device(be._ctx, 0, 1, None) == _lib.ERR_INVALID_ARG
    assert L.cmx_backend_recon_surface_decay_device(be._ctx, 0, 1, None, 1e6, None) == _lib.ERR_INVALID_ARG
    assert L.cmx_backend_recon_surface_decay(be._ctx, 0, 1, None, 1e6, None) == _lib.ERR_INVALID_ARG
    # a bad tau
    for tau in (0.0, -1.0, nan, inf, -inf):
        assert status_of(hip, be.reconstruct_surface_decay, tau) == _lib.ERR_INVALID_ARG, tau
    counts_only = np.zeros(3, np.int64)
    assert L.cmx_backend_recon_surface_get(be._ctx, 0, 3, None, counts_only.ctypes.data_as(_lib.c_i64p)) == _lib.OK
    assert np.array_equal(counts_only, snap[1])
    untouched()
    be.reconstruct_end()
    store.close()
    bare.close()


# ---------------------------------------------------------------- 7. example
def test_example_writes_one_npy_of_time_surfaces(hip, tmp_path):
    import os
    import sys
    from cmax_slam_amd import synth
    ex = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples")
    if ex not in sys.path:
        sys.path.insert(0, ex)
    import rotation_pipeline as rp
    stream = synth.event_stream(2e6, 0.5, 240, 180, 200.0, 200.0, 119.5, 89.5, omega_mean=(0.2, 1.8, 0.3), omega_amp=(1.0, 0.8, 1.0), seed=77)
    path = str(tmp_path / "surfaces.npy")
    res = rp.run_pipeline(stream, rp.Params(), time_surfaces=path, surface_ms=50.0)
    decayed, counts = res["time_surfaces"]
    on_disk = np.load(path)
    print("example: %s surfaces, %s events each" % (decayed.shape, counts.tolist()))
    assert on_disk.shape == decayed.shape == (len(counts), 2, 180, 240) and len(counts) >= 5 and on_disk.dtype == np.float32
    assert on_disk.tobytes() == decayed.tobytes()
    assert (counts > 0).all()  # no surface inside the recording is empty
    assert (on_disk >= 0.0).all() and (on_disk <= 1.0).all()
    assert (on_disk > 0).any(axis=(2, 3)).all()  # both channels of every surface are non-zero
    text = open(os.path.join(ex, "rotation_pipeline.py")).read()
    assert "--time-surfaces" in text and "--surface-ms" in text and "--surface-tau-ms" in text
