"""GPU: per-event support scores (cmx_backend_recon_score* / BackendEvaluator.reconstruct_score*): the panorama read back at every
event, with or without the event's own vote.

The main checks need no tolerance: a score is fp32 arithmetic in a stated order on values a host can fetch -- the support plane
(reconstruct_score_plane, at sigma 0 reconstruct_get) and the exported coordinates (reconstruct_warp) -- so the fp32 emulation of
tests/recon_score_cases.py on the device's OWN plane and coordinates must give the device's scores BIT FOR BIT, every event compared.
Beside them: the independent reference (reference coordinates on the oracle's plane), S and the own contribution at sigma 1 and 2
against the dense fp64 operators of tests/dense_image_ops.py -- on two configurations whose votes reach all four borders --, the
sum identity, the ingest paths and internal slices, the lone trailing event, states and errors, and that the pass only reads.

Tolerances.  Independent reference, per event: 4 x (RTOL x max |oracle plane|: the plane tolerance of tests/test_gpu_recon.py, four
cells) + PARITY_BOUND of tests/test_gpu_recon_warp.py x (sum of the four absolute cell differences around the event: what a shift of
the coordinate moves) + 8 x 2^-24 x sum w |S| (the seven roundings of the score).  S: 8 max(e32, 2^-24) max |ref|, the rule of
dense_image_ops.bound.  Own contribution: 32 x 2^-24 relative (positive terms, about sixteen roundings, doubled) + one ulp of the
score (it is read as a difference of two scores).  Sum identity: 2^-20 relative (seven roundings per positive term, doubled)."""
import numpy as np
import pytest

import dense_image_ops as dio
import recon_cases as rc
import recon_score_cases as sc
import recon_warp_cases as wc
from cmax_slam_amd import _lib
from test_gpu_recon_warp import PARITY_BOUND
from util import RTOL

pytestmark = pytest.mark.gpu
W, H = rc.SENSOR[:2]
MODES = (False, True)  # deterministic
SMOOTH = ("A", "poles") + tuple(sc.BORDER)


def make(hip, name, deterministic=False):
    c, w = sc.case(name)[:2]
    be = hip.BackendEvaluator(W, H, w.lut, c["Wp"], c["Hp"])
    if deterministic:
        be.set_deterministic(True)
    return be


def begin(be, name):
    c, w, _, _, _, knots = sc.case(name)
    be.reconstruct_begin(c["order"], knots, w.start_ns, w.dt_ns, c["batch"], c["rate"])


def store_of(hip, name):
    x, y, t = sc.case(name)[2:5]
    store = hip.EventStore(W, H, max(len(x), 1))
    if len(x):
        store.push(x, y, t)
    return store


def opened(hip, name, deterministic=False, sigma=0.0, n_add=None):
    """(be, store) with the configuration's events added (the first n_add of them) and a score pass open at sigma"""
    be, store = make(hip, name, deterministic), store_of(hip, name)
    begin(be, name)
    be.reconstruct_add_from(store, 0, sc.case(name)[0]["N"] if n_add is None else n_add)
    be.reconstruct_score_open(sigma)
    return be, store


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint8)


def same(a, b):
    return a[0].dtype == b[0].dtype == np.float32 and a[0].shape == b[0].shape and a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


def status_of(hip, fn, *a, **k):
    with pytest.raises(hip.CmaxHipError) as e:
        fn(*a, **k)
    return e.value.status


def ulp32(v):
    return np.spacing(np.abs(np.asarray(v, np.float32))).astype(np.float64)


# ---------------------------------------------------------------- 1. + 2. bitwise closure and leave-one-out at sigma 0
@pytest.mark.parametrize("deterministic", MODES)
@pytest.mark.parametrize("name", wc.CLOSURE)
def test_sigma0_scores_are_the_emulation_on_the_devices_own_plane(hip, name, deterministic):
    n = sc.case(name)[0]["N"]
    be, store = opened(hip, name, deterministic)
    s0, fl = be.reconstruct_score_from(store, 0, n, loo=False)
    s1, fl1 = be.reconstruct_score_from(store, 0, n, loo=True)
    plane = be.reconstruct_get()
    xy, wfl = be.reconstruct_warp_from(store, 0, n)
    S = be.reconstruct_score_plane()
    be.reconstruct_end()
    store.close()
    assert s0.shape == (n,) and s0.dtype == np.float32 and fl.shape == (n,) and fl.dtype == np.uint8
    assert fl.tobytes() == wfl.tobytes() == fl1.tobytes()
    assert S.tobytes() == plane.tobytes()
    emu = sc.score32(plane, xy[:, 0], xy[:, 1], wfl)
    d0 = int(np.count_nonzero(bits(s0) != bits(emu)))
    want1 = sc.loo32(emu, sc.self0_32(xy[:, 0], xy[:, 1]), wfl)
    d1 = int(np.count_nonzero(bits(s1) != bits(want1)))
    print("%s %s: %d events, %d voted; scores that differ in bits: %d (loo off), %d (loo on); loo min %.3e" %
          (name, "deterministic" if deterministic else "default", n, int((wfl == 3).sum()), d0, d1, float(s1.min())))
    assert (wfl == 3).sum() > 0 and float(s0.max()) > 0
    assert d0 == 0
    assert d1 == 0
    assert (s1[wfl != 3] == s0[wfl != 3]).all() and (s0[(wfl & 2) == 0] == 0).all()


@pytest.mark.parametrize("deterministic", MODES)
def test_two_events_alone_in_their_cells_score_zero(hip, deterministic):
    name = "n2"
    c, w, _, _, t, knots = sc.case(name)
    x, y = np.array([20, 200], np.uint16), np.array([20, 150], np.uint16)
    be = make(hip, name, deterministic)
    begin(be, name)
    be.reconstruct_add(x, y, t)
    be.reconstruct_score_open(0.0)
    s0, fl = be.reconstruct_score(x, y, t, loo=False)
    s1, _ = be.reconstruct_score(x, y, t, loo=True)
    xy, _ = be.reconstruct_warp(x, y, t)
    be.reconstruct_end()
    assert (fl == 3).all() and np.abs(np.trunc(xy[0]) - np.trunc(xy[1])).max() >= 2  # (both voted, into disjoint cells)
    print("two lone events, %s: scores %s, leave-one-out %s" % ("deterministic" if deterministic else "default", s0, s1))
    assert (s0 > 0.25).all()  # (sum of four squared weights that add up to one)
    if deterministic:
        assert (np.abs(s1.astype(np.float64)) <= 2.0 ** -28).all()  # (the plane is quantised to 2^-30 per vote, four cells)
    else:
        assert s1.tobytes() == np.zeros(2, np.float32).tobytes()


# ---------------------------------------------------------------- 3. sum identity
@pytest.mark.parametrize("name", ["A", "B", "poles"])
def test_sum_of_voting_scores_is_the_sum_of_squares(hip, name):
    c = sc.case(name)[0]
    be, store = opened(hip, name)
    s0, fl = be.reconstruct_score_from(store, 0, c["N"], loo=False)
    plane = be.reconstruct_get()
    ms = be.reconstruct_contrast(0.0, _lib.MEAN_SQUARE)
    again = be.reconstruct_score_from(store, 0, c["N"], loo=False)  # (contrast does not close the pass)
    be.reconstruct_end()
    store.close()
    lhs = float(s0[fl == 3].sum(dtype=np.float64))
    rhs = float((plane.astype(np.float64) ** 2).sum())
    print("%s: sum score %.9e, sum plane^2 %.9e (rel %.2e), Wp Hp mean square %.9e" % (name, lhs, rhs, abs(lhs - rhs) / rhs, c["Wp"] * c["Hp"] * ms))
    assert rhs > 0 and abs(lhs - rhs) <= 2.0 ** -20 * rhs
    assert abs(lhs - c["Wp"] * c["Hp"] * ms) <= (2.0 ** -20 + 1e-9) * rhs
    assert same(again, (s0, fl))


# ---------------------------------------------------------------- 4. independent reference
@pytest.mark.parametrize("sigma", (0.0,) + sc.SIGMAS)
@pytest.mark.parametrize("name", ["A", "B", "poles", "pano130x96"] + list(sc.BORDER))
def test_against_the_reference_coordinates_on_the_oracle_plane(hip, oracle, name, sigma):
    c = sc.case(name)[0]
    be, store = opened(hip, name, sigma=sigma)
    s0, fl = be.reconstruct_score_from(store, 0, c["N"], loo=False)
    be.reconstruct_end()
    store.close()
    px, py, fl_ref = sc.reference(name)
    P = sc.oracle_plane(name)
    S = sc.support_ref(P, sigma)
    keep = ~wc.near_integer(px, py)
    assert np.count_nonzero(~keep) <= wc.MAX_NEAR_INTEGER
    np.testing.assert_array_equal(fl[keep], fl_ref[keep])
    m = keep & ((fl_ref & wc.INSIDE) != 0)
    xx, yy, dx, dy = sc.cells(px[m], py[m])
    w = sc.iwe_numpy._weights(dx, dy).astype(np.float64)
    s00, s01, s10, s11 = S[yy, xx], S[yy, xx + 1], S[yy + 1, xx], S[yy + 1, xx + 1]
    ref = w[:, 0] * s00 + w[:, 1] * s01 + w[:, 2] * s10 + w[:, 3] * s11
    tol = (4 * RTOL * float(np.abs(P).max()) + PARITY_BOUND * (np.abs(s01 - s00) + np.abs(s11 - s10) + np.abs(s10 - s00) + np.abs(s11 - s01))
           + 8 * 2.0 ** -24 * (w[:, 0] * np.abs(s00) + w[:, 1] * np.abs(s01) + w[:, 2] * np.abs(s10) + w[:, 3] * np.abs(s11)))
    err = np.abs(s0[m].astype(np.float64) - ref)
    k = int(np.argmax(err / tol))
    print("%s sigma %g: %d events compared, max |score - ref| %.3e (largest score %.3f), worst error / tolerance %.3f" %
          (name, sigma, int(m.sum()), float(err.max()), float(ref.max()), float(err[k] / tol[k])))
    assert m.sum() > 1000 and (err <= tol).all()
    assert (s0[keep & ((fl_ref & wc.INSIDE) == 0)] == 0).all()


# ---------------------------------------------------------------- 5. sigma 1 and 2: S, scores, the own contribution, empty tiles
@pytest.mark.parametrize("sigma", sc.SIGMAS)
@pytest.mark.parametrize("name", SMOOTH)
def test_smoothed_support_scores_and_self_term(hip, oracle, name, sigma):
    c = sc.case(name)[0]
    Hp, Wp, n = c["Hp"], c["Wp"], c["N"]
    be, store = opened(hip, name, sigma=sigma)
    S = be.reconstruct_score_plane()
    plane = be.reconstruct_get()
    s0, fl = be.reconstruct_score_from(store, 0, n, loo=False)
    s1, _ = be.reconstruct_score_from(store, 0, n, loo=True)
    xy, wfl = be.reconstruct_warp_from(store, 0, n)
    be.reconstruct_end()
    store.close()
    # S against the dense operators on the device's plane
    ref = dio.blurred(plane, sigma)
    bound, e32 = sc.support_bound(plane, sigma, ref)
    errS = float(np.abs(S.astype(np.float64) - ref).max())
    print("%s sigma %g: max |S - ref| %.3e, bound %.3e (e32 %.2e, max |ref| %.3f)" % (name, sigma, errS, bound, e32, float(np.abs(ref).max())))
    assert errS <= bound
    # scores: the emulation on the device's own S, bit for bit
    assert fl.tobytes() == wfl.tobytes()
    emu = sc.score32(S, xy[:, 0], xy[:, 1], wfl)
    d0 = int(np.count_nonzero(bits(s0) != bits(emu)))
    print("   %d events, scores that differ from the emulation in bits: %d" % (n, d0))
    assert d0 == 0
    assert (s1[wfl != 3] == s0[wfl != 3]).all()
    # the own contribution against w^T (Gy (x) Gx) w of the dense operators
    m = wfl == 3
    got = s0[m].astype(np.float64) - s1[m].astype(np.float64)
    want = sc.self_ref(xy[m, 0], xy[m, 1], Hp, Wp, sigma)
    tol = 32 * 2.0 ** -24 * want + ulp32(s0[m])
    _, fold = sc.self_closed(xy[m, 0], xy[m, 1], Hp, Wp, sigma)
    err = np.abs(got - want)
    k = int(np.argmax(err / tol))
    print("   own contribution: %d voting events (%s with a fold left / right / top / bottom), worst error / tolerance %.3f at a self of %.4f" %
          (int(m.sum()), fold.sum(axis=0), float(err[k] / tol[k]), float(want[k])))
    assert (err <= tol).all()
    if name in sc.BORDER:
        assert (fold.sum(axis=0) >= sc.MIN_FOLDED).all()


@pytest.mark.parametrize("name,half", [("A", 30_000), ("sweep256x128", 20_000)])
def test_support_is_zero_where_no_vote_reaches(hip, name, half):
    """the first half of the stream is added, the second half scored: S is exactly zero on every tile without a vote within the
    radius (whatever an earlier pass left there), and an event whose four cells lie there scores exactly zero"""
    c, _, x, y, t, _ = sc.case(name)
    sigma = 1.0
    r = dio.radius(sigma)
    be, store = opened(hip, name, sigma=sigma)        # an earlier pass over ALL events: S is non-zero wherever any of them reaches
    be.reconstruct_restart(sc.case(name)[5])          # closes the pass and zeroes the plane; the support plane keeps what it held
    be.reconstruct_add_from(store, 0, half)
    be.reconstruct_score_open(sigma)
    S = be.reconstruct_score_plane()
    plane = be.reconstruct_get()
    # (loo off: these events did not vote, and leave-one-out subtracts an own contribution by the flags alone)
    s0, fl = be.reconstruct_score(x[half:], y[half:], t[half:], loo=False)
    xy, _ = be.reconstruct_warp(x[half:], y[half:], t[half:])
    be.reconstruct_end()
    store.close()
    active = dio.compare_set(plane, r, reach=r)
    assert (S[~active] == 0).all()
    inside = (fl & 2) != 0
    xx, yy = sc.cells(xy[inside, 0], xy[inside, 1])[:2]
    empty = ~(active[yy, xx] | active[yy, xx + 1] | active[yy + 1, xx] | active[yy + 1, xx + 1])
    print("%s: %d of %d pixels on tiles no vote reaches; %d of %d scored events land there" %
          (name, int((~active).sum()), active.size, int(empty.sum()), int(inside.sum())))
    assert (~active).sum() > 0
    assert (s0[inside][empty] == 0).all()
    if name in sc.BORDER:  # (the sweep moves on: its second half lands where the first never was)
        assert empty.sum() > 100
    assert (fl & 1).all() or c["rate"] > 1  # (scored in cuts of their own: flags are those of THIS call)


# ---------------------------------------------------------------- 6. reproducibility and paths
@pytest.mark.parametrize("deterministic", MODES)
@pytest.mark.parametrize("name,sigma", [("A", 1.0), ("B", 0.0), ("n65", 0.0)])
def test_paths_and_slices_give_the_same_bytes(hip, name, sigma, deterministic):
    import torch
    c, _, x, y, t, _ = sc.case(name)
    n = c["N"]
    be, store = opened(hip, name, deterministic, sigma)
    L = _lib.lib()
    for loo in (False, True):
        want = be.reconstruct_score_from(store, 0, n, loo=loo)
        assert same(be.reconstruct_score(x, y, t, loo=loo), want)
        assert same(be.reconstruct_score_aos(_lib.dvs_events(x, y, t), loo=loo), want)
        d_s = torch.full((n,), -7.0, dtype=torch.float32, device="cuda")
        d_f = torch.full((n,), 99, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()  # (the fills run on torch's stream, the scores on the context's)
        out = be.reconstruct_score_from(store, 0, n, loo=loo, out=(d_s, d_f))
        assert out[0] is d_s and out[1] is d_f
        torch.cuda.synchronize()
        assert same((d_s.cpu().numpy(), d_f.cpu().numpy()), want)
        d_s.fill_(-7.0)
        torch.cuda.synchronize()
        be.reconstruct_score_from(store, 0, n, loo=loo, out=(d_s, None))
        torch.cuda.synchronize()
        assert d_s.cpu().numpy().tobytes() == want[0].tobytes()
        try:
            for n_slice in (1000, 4096):
                assert L.cmx_diag_set(_lib.DIAG_RECON_SLICE_EVENTS, n_slice) == 0
                assert same(be.reconstruct_score_from(store, 0, n, loo=loo), want), n_slice
                assert same(be.reconstruct_score(x, y, t, loo=loo), want), n_slice
        finally:
            assert L.cmx_diag_set(_lib.DIAG_RECON_SLICE_EVENTS, 0) == 0
    # a sub-range off the batch grid is a call of its own: batches start at its first event
    lo, m = 7 * 64 + 1, 5 * 64 + 1
    if n >= lo + m:
        assert same(be.reconstruct_score_from(store, lo, m, loo=False), be.reconstruct_score(x[lo:lo + m], y[lo:lo + m], t[lo:lo + m], loo=False))
    be.reconstruct_end()
    store.close()


def test_two_deterministic_runs_are_bitwise_equal(hip):
    name = "A"
    n = sc.case(name)[0]["N"]
    runs = []
    for _ in range(2):
        be, store = opened(hip, name, True, 1.0)
        runs.append((be.reconstruct_score_from(store, 0, n, loo=True), be.reconstruct_score_plane()))
        be.reconstruct_end()
        store.close()
    assert same(runs[0][0], runs[1][0]) and runs[0][1].tobytes() == runs[1][1].tobytes()


# ---------------------------------------------------------------- 7. the lone trailing event
@pytest.mark.parametrize("name", ["n65", "n1"])
def test_lone_trailing_event(hip, oracle, name):
    c, _, x, y, t, _ = sc.case(name)
    n = c["N"]
    be = make(hip, name)
    begin(be, name)
    be.reconstruct_add(x, y, t)
    # more support under the lone event than its own vote could explain: every event once more, as batches of their own
    if n > 1:
        be.reconstruct_add(x[:n - 1], y[:n - 1], t[:n - 1])
    be.reconstruct_score_open(0.0)
    s0, fl = be.reconstruct_score(x, y, t, loo=False)
    s1, _ = be.reconstruct_score(x, y, t, loo=True)
    plane = be.reconstruct_get()
    xy, wfl = be.reconstruct_warp(x, y, t)
    be.reconstruct_end()
    px, py, fl_ref = sc.reference(name)
    assert fl.tobytes() == wfl.tobytes() == fl_ref.tobytes()
    assert fl[n - 1] & 1 == 0 and fl[n - 1] & 2  # SAMPLED clear, inside
    assert abs(xy[n - 1, 0] - px[n - 1]) <= PARITY_BOUND and abs(xy[n - 1, 1] - py[n - 1]) <= PARITY_BOUND  # its own time's pose
    emu = sc.score32(plane, xy[:, 0], xy[:, 1], wfl)
    assert bits(s0).tobytes() == bits(emu).tobytes()
    assert s1[n - 1] == s0[n - 1]  # nothing is subtracted: it did not vote
    if n > 1:
        assert (s1[:n - 1] < s0[:n - 1]).all()


# ---------------------------------------------------------------- 8. state and errors
def test_states_and_errors(hip):
    name = "window"
    c, w, x, y, t, knots = sc.case(name)
    n = c["N"]
    L = _lib.lib()
    be, store = make(hip, name), store_of(hip, name)
    sco, fl = np.full(n + 1, -7.0, np.float32), np.full(n + 1, 99, np.uint8)

    def raw(ctx, x, y, t, count=None, out=sco):
        return L.cmx_backend_recon_score(ctx, len(x) if count is None else count, x.ctypes.data_as(_lib.c_u16p), y.ctypes.data_as(_lib.c_u16p),
                                         t.ctypes.data_as(_lib.c_i64p), 1, out.ctypes.data if out is not None else None, fl.ctypes.data)

    def raw_from(ctx, st, first, count):
        return L.cmx_backend_recon_score_from(ctx, st._h, first, count, 1, sco.ctypes.data, fl.ctypes.data)

    def untouched():
        assert (sco == -7.0).all() and (fl == 99).all()

    # before begin, on a group handle, before score_open
    assert raw(be._ctx, x, y, t) == _lib.ERR_STATE and raw_from(be._ctx, store, 0, n) == _lib.ERR_STATE
    assert status_of(hip, be.reconstruct_score_open, 0.0) == _lib.ERR_STATE
    assert status_of(hip, be.reconstruct_score_plane) == _lib.ERR_STATE
    grp = hip.BackendEvaluator(W, H, w.lut, c["Wp"], c["Hp"], devices=[0, 0], transport=_lib.GROUP_DIRECT)
    assert raw(grp._ctx, x, y, t) == _lib.ERR_STATE and status_of(hip, grp.reconstruct_score_open, 0.0) == _lib.ERR_STATE
    grp.close()
    begin(be, name)
    assert raw(be._ctx, x, y, t) == _lib.ERR_STATE and raw_from(be._ctx, store, 0, n) == _lib.ERR_STATE
    assert status_of(hip, be.reconstruct_score_aos, _lib.dvs_events(x, y, t)) == _lib.ERR_STATE
    assert status_of(hip, be.reconstruct_score_plane) == _lib.ERR_STATE
    assert L.cmx_backend_recon_score_from_device(be._ctx, store._h, 0, n, 1, None, None) == _lib.ERR_STATE
    untouched()
    # what closes the pass
    be.reconstruct_add_from(store, 0, n)
    for close in (lambda: be.reconstruct_add(x[:200], y[:200], t[:200]), lambda: be.reconstruct_restart(knots),
                  lambda: (be.reconstruct_bind(store, 0, n), be.reconstruct_score_open(1.0), be.reconstruct_eval_bound(None, 1.0)),
                  lambda: be.reconstruct_extend(knots), lambda: be.reconstruct_eval(store, 0, n, None, 1.0, want_grad=False)):
        be.reconstruct_score_open(1.0)
        assert raw_from(be._ctx, store, 0, 10) == 0
        close()
        assert raw_from(be._ctx, store, 0, n) == _lib.ERR_STATE and raw(be._ctx, x, y, t) == _lib.ERR_STATE
        assert status_of(hip, be.reconstruct_score_plane) == _lib.ERR_STATE
    sco[:], fl[:] = -7.0, 99
    # what does not
    be.reconstruct_add_from(store, 0, n)
    be.reconstruct_score_open(1.0)
    want = be.reconstruct_score_from(store, 0, n)
    S = be.reconstruct_score_plane()
    pol = (np.arange(n) % 2).astype(np.uint8)
    be.reconstruct_pol_add(x, y, t, pol)
    be.reconstruct_view_begin([_lib.recon_view((0, 0, 0, 1), 100.0, 100.0, 32.0, 24.0, int(t[0]), int(t[-1]) + 1)], 64, 48)
    be.reconstruct_view_add(x, y, t)
    be.reconstruct_warp(x, y, t)
    be.reconstruct_get()
    be.reconstruct_render()
    be.reconstruct_contrast(2.0)  # (another sigma: the pass has its own taps)
    assert same(be.reconstruct_score_from(store, 0, n), want) and be.reconstruct_score_plane().tobytes() == S.tobytes()
    # arguments of score_open: refused, and the open pass is as it was
    assert status_of(hip, be.reconstruct_score_open, float("nan")) == _lib.ERR_INVALID_ARG
    assert status_of(hip, be.reconstruct_score_open, float("inf")) == _lib.ERR_INVALID_ARG
    assert status_of(hip, be.reconstruct_score_open, 3.5) == _lib.ERR_INVALID_ARG  # radius 14 > 12
    assert same(be.reconstruct_score_from(store, 0, n), want)
    # NULL output, counts
    assert raw(be._ctx, x, y, t, out=None) == _lib.ERR_INVALID_ARG
    assert L.cmx_backend_recon_score_from_device(be._ctx, store._h, 0, n, 1, None, None) == _lib.ERR_INVALID_ARG
    assert raw_from(be._ctx, store, 0, n + 1) == _lib.ERR_INVALID_ARG and raw(be._ctx, x, y, t, count=-1) == _lib.ERR_INVALID_ARG
    assert raw(be._ctx, x, y, t, count=0) == 0 and raw(be._ctx, x, y, t, count=0, out=None) == 0 and raw_from(be._ctx, store, 0, 0) == 0
    untouched()
    # warp*'s validation, complete before anything is written
    bad_x = x.copy()
    bad_x[-2] = W
    assert raw(be._ctx, bad_x, y, t) == _lib.ERR_EVENT_RANGE
    back = t.copy()
    back[19_900] = t[19_999] + 1000
    assert raw(be._ctx, x, y, back) == _lib.ERR_TIME_ORDER
    st = hip.EventStore(W, H, n)
    st.push(x, y, back)
    assert raw_from(be._ctx, st, 0, n) == _lib.ERR_TIME_ORDER
    st.close()
    only_tail = t.copy()
    only_tail[-150:] += 10_000_000_000
    assert raw(be._ctx, x, y, only_tail) == _lib.ERR_SPLINE_RANGE
    x1, y1, t1 = np.append(x, x[-1]), np.append(y, y[-1]), np.append(t, t[-1] + 10_000_000_000)
    assert n % c["batch"] == 0
    assert raw(be._ctx, x1, y1, t1) == _lib.ERR_SPLINE_RANGE  # the lone trailing event's own time: warp*'s stricter check
    st = hip.EventStore(W, H, n + 1)
    st.push(x1, y1, t1)
    assert raw_from(be._ctx, st, 0, n + 1) == _lib.ERR_SPLINE_RANGE and raw_from(be._ctx, st, n, 1) == _lib.ERR_SPLINE_RANGE
    untouched()
    assert raw_from(be._ctx, st, 0, n) == 0  # ... and the same input without that event is fine, which the guards show as written
    st.close()
    assert sco[:n].tobytes() == want[0].tobytes() and sco[n] == -7.0 and fl[:n].tobytes() == want[1].tobytes() and fl[n] == 99
    be.reconstruct_end()
    store.close()
    # a panorama that does not hold a single reflection of the kernel: 2r + 1 = 9 >= Hp
    small = hip.BackendEvaluator(W, H, w.lut, 64, 8)
    small.reconstruct_begin(c["order"], knots, w.start_ns, w.dt_ns, c["batch"], c["rate"])
    small.reconstruct_score_open(0.0)
    assert status_of(hip, small.reconstruct_score_open, 1.0) == _lib.ERR_INVALID_ARG
    small.reconstruct_end()


# ---------------------------------------------------------------- 9. read-only
def test_the_score_pass_changes_nothing(hip):
    name = "window"
    c, w, x, y, t, knots = sc.case(name)
    n = c["N"]
    sigma = 1.0

    def run(bracket):
        be, store = make(hip, name, deterministic=True), store_of(hip, name)
        begin(be, name)
        be.reconstruct_add_from(store, 0, n)
        be.reconstruct_contrast(sigma, want_grad=True)
        be.reconstruct_grad_add_from(store, 0, 10_000)
        state = be.reconstruct_get(with_counts=True)
        if bracket:
            be.reconstruct_score_open(sigma)
            assert float(be.reconstruct_score_from(store, 0, n)[0].max()) > 0
            be.reconstruct_score(x, y, t, loo=False)
        be.reconstruct_grad_add_from(store, 10_000, n - 10_000)
        grad = be.reconstruct_grad_get()  # (CMX_ERR_STATE had the score pass closed the gradient pass or touched its counts)
        now = be.reconstruct_get(with_counts=True)
        assert now[0].tobytes() == state[0].tobytes() and now[1:] == state[1:]
        return be, store, grad

    ref_be, ref_store, ref_grad = run(False)
    ref_be.reconstruct_end()
    ref_store.close()
    be, store, grad = run(True)
    assert np.abs(grad).max() > 0 and grad.tobytes() == ref_grad.tobytes()
    # an open gradient pass at ANOTHER sigma is closed, as recon_contrast at that sigma would close it
    be.reconstruct_score_open(2.0)
    assert status_of(hip, be.reconstruct_grad_get) == _lib.ERR_STATE
    # a binding with a frozen, then released head: the pass reads the plane the last evaluation left and the knots
    be.reconstruct_bind(store, 0, n)
    be.reconstruct_eval_bound(None, sigma)
    be.reconstruct_freeze_head(5)
    ev = be.reconstruct_eval_bound(None, sigma)
    be.reconstruct_release_head()
    infos = (be.reconstruct_bound_info(), be.reconstruct_frozen_info(), be.reconstruct_online_info())
    assert infos[2]["released_sampled"] > 0
    state = be.reconstruct_get(with_counts=True)
    be.reconstruct_score_open(0.0)
    s0, fl = be.reconstruct_score_from(store, 0, n, loo=False)
    xy, wfl = be.reconstruct_warp_from(store, 0, n)
    assert fl.tobytes() == wfl.tobytes()
    assert bits(s0).tobytes() == bits(sc.score32(state[0], xy[:, 0], xy[:, 1], wfl)).tobytes() and float(s0.max()) > 0
    assert (be.reconstruct_bound_info(), be.reconstruct_frozen_info(), be.reconstruct_online_info()) == infos
    now = be.reconstruct_get(with_counts=True)
    assert now[0].tobytes() == state[0].tobytes() and now[1:] == state[1:]
    ev2 = be.reconstruct_eval_bound(None, sigma)
    assert ev2[0] == ev[0] and ev2[1].tobytes() == ev[1].tobytes()
    be.reconstruct_end()
    store.close()


# ---------------------------------------------------------------- 10. example
def test_example_scores_the_events(hip, tmp_path):
    import os
    import sys
    from cmax_slam_amd import synth
    ex = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples")
    if ex not in sys.path:
        sys.path.insert(0, ex)
    import rotation_pipeline as rp
    stream = synth.event_stream(2e6, 0.5, 240, 180, 200.0, 200.0, 119.5, 89.5, omega_mean=(0.2, 1.8, 0.3), omega_amp=(1.0, 0.8, 1.0), seed=77)
    path = str(tmp_path / "scores")
    res = rp.run_pipeline(stream, rp.Params(), score_events=path, score_sigma=1.0)
    z = np.load(path + ".npz")
    s, fl = z["score"], z["flags"]
    assert s.dtype == np.float32 and fl.dtype == np.uint8 and s.shape == fl.shape and len(s) > 0.5 * len(stream.t_ns)
    assert np.isfinite(s).all() and (s[(fl & 2) == 0] == 0).all() and float(s.max()) > 1.0
    assert res["recon"].shape[0] > 0
    assert "--score-events" in open(os.path.join(ex, "rotation_pipeline.py")).read()
