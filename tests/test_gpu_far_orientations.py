"""-m gpu: the back-end warp away from the panorama's centre -- at the +-pi seam, at the pole rows and behind the camera -- where
every other back-end test's windows (|phi|, |theta| of a few tenths of a radian) never go.  Inputs: tests/far_cases.py, checked on
the CPU by tests/test_far_cases_cpu.py.

1. Per-event votes.  Probe tables whose 2 x 2 vote cells are disjoint: the plane IS the list of votes, and each cell is held to
   the longdouble projection under the R the device itself reports (get_pose_table) within 4e-7 absolute (three fp32 roundings per
   factor pair: 5 * 2^-24 = 3e-7; the fixed-point forms add 2^-31), every other pixel to exactly 0.  Through be_splat_kernel
   (reference-shaped), be_bin_hist_kernel / be_splat_lds_kernel (production, also deterministic), recon_votes_kernel
   (reconstruct) and recon_votes_lds_kernel (bound).  On the sorted paths the counter looked at is the share of voting events
   that left their tile's LDS window and took the global-atomic path (stats()["fallback_frac"], reconstruct_bound_info()): with
   the sort made at the evaluation's own parameters it must be exactly 0 -- a wrong tile key would be a vote outside its window,
   which the global path would otherwise quietly repair.
2. Per-event derivative planes (be_splat_kernel's DERIV == 1 form) against the oracle's, per cell, relative to the cell's own
   largest magnitude over the P planes (near the poles the phi row is 50 times the equator's).
3. Far windows: test_gpu_backend.py's rules (planes, derivative planes, contrast_fdf / contrast_f at RTOL) on the reference-shaped
   path, test_gpu_exact_arbiter.py's rule on the production path (be_gather*_kernel's fp32 Jacobian, DERIV == 2, at the poles),
   bit-for-bit repeats in deterministic mode, a global map (tile flags, sparse lists, alpha compose at the seam and the pole
   rows), and one context moved centre -> far side -> centre.
Every case prints its figures ("FAR|" lines; profiles/far_orientations.txt is a record of them)."""
import dataclasses

import numpy as np
import pytest

import far_cases as fc
from cmax_slam_amd import _lib
from util import RTOL, rel_img, rel_scalar, rel_vec

pytestmark = pytest.mark.gpu
VOTE_TOL = 4e-7


def _set_probe_window(be, tab, old, num_fixed=1):
    start_ns, dt_ns, t_next = tab.window_args(old)
    be.set_window(tab.x, tab.y, tab.t_ns, 2, tab.knots, start_ns, dt_ns, num_fixed, t_next, fc.BATCH, 1, 0.0, 0)


def _window_form(hip, form, tab):
    be = (hip.reference_shaped.BackendEvaluator if form == "reference-shaped" else hip.BackendEvaluator)(
        fc.SENSOR, fc.SENSOR, tab.lut, tab.Wp, tab.Hp)
    if form != "reference-shaped":
        be.set_fast_path()
        be.set_deterministic(form == "deterministic")
    return be


@pytest.mark.parametrize("Wp,Hp", fc.PANOS)
@pytest.mark.parametrize("name,z1", fc.PROBE_CASES)
def test_per_event_votes(hip, Wp, Hp, name, z1):
    tab, _ = fc.probe_case(Wp, Hp, name, z1)
    worst = {}
    ref = R = None
    for form in ("reference-shaped", "production", "deterministic"):
        be = _window_form(hip, form, tab)
        for old in (True, False):
            _set_probe_window(be, tab, old)
            be.eval(np.zeros(3))
            if ref is None:   # the rotation the device uses: one per batch, all of them Q
                R = be.get_pose_table()[0]
                assert len(R) == -(-tab.n // fc.BATCH) and all(np.array_equal(R[0], r) for r in R)
                R = R[0]
                assert np.abs(R - tab.Q.as_matrix()).max() < 1e-14
                ref = fc.probe_reference(tab.bearings, R, Wp, Hp, tab.n_pole)   # (asserts disjoint cells, distance >= 1e-7)
            mine, other = (_lib.PLANE_IL_OLD, _lib.PLANE_IL_NEW) if old else (_lib.PLANE_IL_NEW, _lib.PLANE_IL_OLD)
            d = fc.compare_plane(tab, ref, R, be.get_plane(mine), VOTE_TOL)
            assert not be.get_plane(other).any(), (form, old)
            worst[form] = max(worst.get(form, 0.0), d)
            if form != "reference-shaped":
                st = be.stats()
                assert st["rebins"] >= 1 and st["fallback_frac"] == 0.0, (form, old, st["rebins"], st["fallback_frac"])
        be.close()
    # whole-trajectory forms: one plane, no old / new split
    start_ns, dt_ns, _ = tab.window_args(True)
    n_kept = int(ref.kept.sum())
    be = hip.BackendEvaluator(fc.SENSOR, fc.SENSOR, tab.lut, Wp, Hp)
    plane = be.reconstruct(tab.x, tab.y, tab.t_ns, 2, tab.knots, start_ns, dt_ns, event_batch_size=fc.BATCH)
    worst["reconstruct"] = fc.compare_plane(tab, ref, R, plane, VOTE_TOL)
    store = hip.EventStore(fc.SENSOR, fc.SENSOR, tab.n)
    store.push(tab.x, tab.y, tab.t_ns)
    be.reconstruct_begin(2, tab.knots, start_ns, dt_ns, fc.BATCH, 1)
    be.reconstruct_bind(store, 0, tab.n)
    be.reconstruct_eval_bound(None, want_grad=False)
    plane, n_sampled, n_inside = be.reconstruct_get(with_counts=True)
    worst["bound"] = fc.compare_plane(tab, ref, R, plane, VOTE_TOL)
    info = be.reconstruct_bound_info()
    assert (n_sampled, n_inside) == (tab.n, n_kept) and info["sorts"] == 1 and info["fallback_frac"] == 0.0, (n_sampled, n_inside, info)
    be.reconstruct_end()
    store.close()
    be.close()
    print("FAR|votes|%dx%d|%s%s|%d kept / %d dropped|" % (Wp, Hp, name, " z1" if z1 else "", n_kept, tab.n - n_kept)
          + " ".join("%s %.2e" % kv for kv in worst.items()))


@pytest.mark.parametrize("Wp,Hp", fc.PANOS)
@pytest.mark.parametrize("name,z1", fc.PROBE_CASES)
def test_per_event_derivative_planes(hip, oracle, Wp, Hp, name, z1):
    tab, ref = fc.probe_case(Wp, Hp, name, z1)
    be = _window_form(hip, "reference-shaped", tab)
    _set_probe_window(be, tab, True, num_fixed=0)
    P = 6
    iwe, planes = be.computeImageOfWarpedEvents(np.zeros(P), want_deriv=True)
    orc = oracle.Backend(fc.SENSOR, fc.SENSOR, tab.lut, Wp, Hp, 2, fc.BATCH, 1, 0.0, 0)
    start_ns, dt_ns, t_next = tab.window_args(True)
    orc.set_window(tab.x, tab.y, tab.t_ns, tab.knots, start_ns, dt_ns, 0, t_next)
    iwe_ref, planes_ref = orc.iwe(np.zeros(P), planes=True)
    assert planes.shape == planes_ref.shape == (P, Hp, Wp) and np.isfinite(planes).all()
    fc.compare_plane(tab, ref, tab.Q.as_matrix(), iwe, VOTE_TOL)
    k = np.flatnonzero(ref.kept)
    ys = ref.yy[k][:, None] + np.array([0, 0, 1, 1])
    xs = ref.xx[k][:, None] + np.array([0, 1, 0, 1])
    got, want = planes[:, ys, xs].astype(np.float64), planes_ref[:, ys, xs].astype(np.float64)    # P x kept x 4
    scale = np.abs(want).max(axis=(0, 2))
    assert scale.min() > 0
    ratio = np.abs(got - want).max(axis=(0, 2)) / scale
    i = int(np.argmax(ratio))
    print("FAR|deriv|%dx%d|%s%s|largest per-cell ratio %.2e (cell scale %.3g .. %.3g)" %
          (Wp, Hp, name, " z1" if z1 else "", ratio[i], scale.min(), scale.max()))
    assert ratio[i] < RTOL, fc.describe(tab, ref, tab.Q.as_matrix(), int(k[i]))
    outside = ~ref.mask
    assert not planes[:, outside].any()       # dropped probes and the poles leave nothing in any derivative plane either
    be.close()


# ---------------------------------------------------------------- far windows
def _oracles(oracle, w, measure, IG=None, exact=True):
    args = (w.W, w.H, w.lut, w.Wp, w.Hp, w.order, w.batch, w.sample_rate, w.sigma, measure)
    win = (w.x, w.y, w.t_ns, w.knots_init, w.start_ns, w.dt_ns, w.num_fixed, w.t_next_win_beg_ns, IG)
    ref = oracle.Backend(*args)
    ref.set_window(*win)
    ex = None
    if exact:
        ex = oracle.BackendExact(*args)
        ex.set_window(*win)
    return ref, ex


def _set(be, w, measure, IG=None):
    be.set_window(w.x, w.y, w.t_ns, w.order, w.knots_init, w.start_ns, w.dt_ns, w.num_fixed, w.t_next_win_beg_ns, w.batch,
                  w.sample_rate, w.sigma, measure, IG)


def _arbiter(tag, got, orc, exact):
    """test_gpu_exact_arbiter.py's rule; returns (contrast vs oracle, contrast vs exact, gradient vs oracle, gradient vs exact)"""
    (c, g), (c_or, g_or), (c_ex, g_ex) = got, orc, exact
    fig = (rel_scalar(c, c_or), rel_scalar(c, c_ex), rel_vec(g, g_or), rel_vec(g, g_ex))
    assert fig[0] < RTOL and fig[1] < RTOL, (tag, fig)
    assert fig[3] < RTOL, (tag, fig)                               # within 1e-5 of the exact value
    if fig[2] >= RTOL:                                             # further than that from the oracle:
        assert rel_vec(g_or, g_ex) > fig[2] - RTOL, (tag, fig)     # the oracle's own rounding
    return fig


@pytest.mark.parametrize("which,name", fc.FAR_CASES)
@pytest.mark.parametrize("measure", [0, 1])
def test_far_window_reference_shaped_path(hip, oracle, which, name, measure):
    w = fc.far_window(which, name)
    ref, _ = _oracles(oracle, w, measure, exact=False)
    be = hip.reference_shaped.BackendEvaluator(w.W, w.H, w.lut, w.Wp, w.Hp)
    _set(be, w, measure)
    drot = np.random.default_rng(3).normal(0, 0.01, w.P)
    iwe, planes = be.computeImageOfWarpedEvents(drot, want_deriv=True)
    iwe_ref, planes_ref = ref.iwe(drot, planes=True)
    fig = [rel_img(be.get_plane(_lib.PLANE_IL_OLD), ref.IL_old), rel_img(be.get_plane(_lib.PLANE_IL_NEW), ref.IL_new),
           rel_img(iwe, iwe_ref), np.abs(planes.astype(np.float64) - planes_ref).max() / np.abs(planes_ref).max()]
    assert ref.IL_old.sum() > 0 and ref.IL_new.sum() > 0
    assert planes.shape == planes_ref.shape
    worst_c = worst_g = 0.0
    for d in fc.far_points(w):
        c_ref, g_ref = ref.eval(d)
        f, df = be.contrast_fdf(d)
        ec, eg, ef = rel_scalar(-f, c_ref), rel_vec(-df, g_ref), rel_scalar(-be.contrast_f(d), c_ref)
        worst_c, worst_g = max(worst_c, ec, ef), max(worst_g, eg)
    print("FAR|window-ref|%s|%s|measure %d|IL_old %.2e IL_new %.2e IWE %.2e derivative planes %.2e contrast %.2e gradient %.2e" %
          (which, name, measure, *fig, worst_c, worst_g))
    assert max(fig) < RTOL
    assert worst_c < RTOL and worst_g < RTOL
    be.close()


@pytest.mark.parametrize("which,name", fc.FAR_CASES)
@pytest.mark.parametrize("measure", [0, 1])
def test_far_window_production_path(hip, oracle, which, name, measure):
    w = fc.far_window(which, name)
    ref, ex = _oracles(oracle, w, measure)
    be = hip.BackendEvaluator(w.W, w.H, w.lut, w.Wp, w.Hp)
    be.set_fast_path()
    _set(be, w, measure)
    worst = np.zeros(4)
    for i, d in enumerate(fc.far_points(w)):
        orc, exact = ref.eval(d), ex.eval(d)
        worst = np.maximum(worst, _arbiter((which, name, measure, i), be.eval(d), orc, exact))
        assert rel_scalar(be.eval(d, want_grad=False)[0], orc[0]) < RTOL
    print("FAR|window-prod|%s|%s|measure %d|contrast vs oracle %.2e vs exact %.2e, gradient vs oracle %.2e vs exact %.2e" %
          (which, name, measure, *worst))
    be.close()
    # deterministic mode: the same bits from a repeated point and from another context, and still the oracle's numbers
    runs = []
    d0, d1 = fc.far_points(w)
    for _ in range(2):
        det = hip.BackendEvaluator(w.W, w.H, w.lut, w.Wp, w.Hp)
        det.set_fast_path()
        det.set_deterministic(True)
        _set(det, w, measure)
        out = [det.eval(d0), det.eval(d1), det.eval(d0)]
        runs.append(out + [(det.get_plane(_lib.PLANE_IL_OLD).tobytes(), np.zeros(0))])
        det.close()
    for (c0, g0), (c1, g1) in zip(runs[0], runs[1]):
        assert c0 == c1 and np.array_equal(g0, g1)
    assert runs[0][0][0] == runs[0][2][0] and np.array_equal(runs[0][0][1], runs[0][2][1])
    _arbiter((which, name, measure, "deterministic"), runs[0][1], ref.eval(d1), ex.eval(d1))


@pytest.mark.parametrize("name", fc.GLOBAL_MAP_FAR)
@pytest.mark.parametrize("measure", [0, 1])
def test_far_window_with_a_global_map(hip, oracle, name, measure):
    """test_gpu_backend.py's test_global_map_and_alpha with the map, the events and the blend at the seam / at the pole rows"""
    w = fc.far_window("linear", name)
    ref0, _ = _oracles(oracle, dataclasses.replace(w, knots_init=w.knots_true), measure, exact=False)
    ref0.iwe(np.zeros(w.P))
    IG = ref0.IL_old.copy() * 1.7
    ref, ex = _oracles(oracle, w, measure, IG)
    be = hip.BackendEvaluator(w.W, w.H, w.lut, w.Wp, w.Hp)
    be.set_fast_path()
    _set(be, w, measure, IG)
    d0, d1 = np.zeros(w.P), np.random.default_rng(8).normal(0, 0.01, w.P)
    fig0 = _arbiter((name, measure, 0), be.eval(d0), ref.eval(d0), ex.eval(d0))
    assert ref.alpha > 0
    ea = rel_scalar(be.alpha, ref.alpha)
    a_first = be.alpha
    fig1 = _arbiter((name, measure, 1), be.eval(d1), ref.eval(d1), ex.eval(d1))   # alpha stays what the first evaluation made it
    assert be.alpha == a_first
    ei = rel_img(be.get_plane(_lib.PLANE_IWE), ref.iwe(d1))
    print("FAR|global-map|%s|measure %d|alpha %.2e IWE %.2e, contrast vs oracle %.2e vs exact %.2e, gradient vs oracle %.2e vs exact %.2e"
          % (name, measure, ea, ei, *np.maximum(fig0, fig1)))
    assert ea < RTOL and ei < RTOL
    be.close()


@pytest.mark.parametrize("with_map", [False, True])
def test_one_context_moves_to_the_far_side_and_back(hip, oracle, with_map):
    """centre window -> yaw 180 window -> centre window on one context: the planes' ping-pong and the tile flags when every
    active tile moves to the other end of the panorama (and, with a map, the compose over both regions)"""
    centre, far = fc.base_window("linear"), fc.far_window("linear", "yaw180")
    IG = None
    if with_map:   # a map that covers both regions: the true trajectories' old halves
        IG = np.zeros((centre.Hp, centre.Wp), np.float32)
        for w in (centre, far):
            r, _ = _oracles(oracle, dataclasses.replace(w, knots_init=w.knots_true), 0, exact=False)
            r.iwe(np.zeros(w.P))
            IG += 1.7 * r.IL_old
    be = hip.BackendEvaluator(centre.W, centre.H, centre.lut, centre.Wp, centre.Hp)
    be.set_fast_path()
    for step, w in enumerate((centre, far, centre)):
        ref, ex = _oracles(oracle, w, 0, IG)
        _set(be, w, 0, IG)
        worst = np.zeros(4)
        for i, d in enumerate(fc.far_points(w)):
            worst = np.maximum(worst, _arbiter((step, i), be.eval(d), ref.eval(d), ex.eval(d)))
            assert rel_img(be.get_plane(_lib.PLANE_IL_OLD), ref.IL_old) < RTOL     # exactly this evaluation's votes
            assert rel_img(be.get_plane(_lib.PLANE_IL_NEW), ref.IL_new) < RTOL
        if with_map:
            assert ref.alpha > 0 and rel_scalar(be.alpha, ref.alpha) < RTOL
        print("FAR|sequence|%s|step %d|contrast vs oracle %.2e vs exact %.2e, gradient vs oracle %.2e vs exact %.2e" %
              ("map" if with_map else "no map", step, *worst))
    be.close()
