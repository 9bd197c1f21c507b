"""GPU: whole-trajectory contrast and its gradient with respect to every control pose (cmx_backend_recon_contrast / _grad_add* /
_grad_get / _eval_from / _restart, BackendEvaluator.reconstruct_*) against the CPU oracle's global_contrast_fdf, for splines longer
than a window can be, every shape at which the gather kernel takes another path, cuts, the three ingest paths, deterministic mode,
the window path, isolation from the evaluation state, the error codes and the refinement built on it.  Evaluation points and oracle
numbers: recon_grad_cases.py (tests/test_recon_grad_inputs_cpu.py shows on the CPU that no comparison is empty and that the oracle
is accurate enough for RTOL at the (case, sigma) pairs used here)."""
import numpy as np
import pytest

import recon_cases as rc
import recon_grad_cases as rg
from cmax_slam_amd import _lib, synth
from util import RTOL, rel_scalar, rel_vec

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
    be.reconstruct_begin(c["order"], rg.point(name) if knots is None else knots, w.start_ns, w.dt_ns, c["batch"], c["rate"])


def feed(be, name, how, pieces, grad, store=None):
    _, x, y, t = rc.window(name)
    for lo, hi in pieces:
        if how == "add":
            (be.reconstruct_grad_add if grad else be.reconstruct_add)(x[lo:hi], y[lo:hi], t[lo:hi])
        elif how == "aos":
            (be.reconstruct_grad_add_aos if grad else be.reconstruct_add_aos)(_lib.dvs_events(x[lo:hi], y[lo:hi], t[lo:hi]))
        else:
            (be.reconstruct_grad_add_from if grad else be.reconstruct_add_from)(store, lo, hi - lo)


def run(be, name, sigma=1.0, measure=0, want_grad=True, how="add", pieces=None, store=None, knots=None):
    """begin at the evaluation point, the vote pass, the image pass, [the gradient pass], end: (contrast, gradient or None)"""
    pieces = pieces or [(0, rc.CASES[name]["N"])]
    begin(be, name, knots)
    feed(be, name, how, pieces, False, store)
    c = be.reconstruct_contrast(sigma, measure, want_grad)
    g = None
    if want_grad:
        feed(be, name, how, pieces, True, store)
        g = be.reconstruct_grad_get()
    be.reconstruct_end()
    return c, g


def check(tag, got, ref):
    (c, g), (cr, gr) = got, ref
    ec, eg = rel_scalar(c, cr), (rel_vec(g, gr) if g is not None else 0.0)
    print("%s: contrast %.8g (oracle %.8g, rel %.2e), gradient rel %.2e, |g|max %.4g" % (tag, c, cr, ec, eg, np.abs(gr).max()))
    assert ec < RTOL
    assert eg < RTOL


@pytest.mark.parametrize("name", ["A", "B"])
@pytest.mark.parametrize("sigma", [1.0, 0.0, 2.0])
def test_long_splines(hip, oracle, name, sigma):
    """A: cubic, K = 100, 60 007 events; B: linear, K = 70, batch 64, rate 3 -- cmx_backend_set_window refuses both splines"""
    be = make(hip, name)
    for measure in (0, 1):
        ref = rg.oracle_ref(oracle, name, sigma, measure)
        check("%s sigma %g measure %d" % (name, sigma, measure), run(be, name, sigma, measure), ref)
        c, _ = run(be, name, sigma, measure, want_grad=False)
        assert rel_scalar(c, ref[0]) < RTOL
    if sigma == 1.0:
        check("%s measure 7 = variance" % name, run(be, name, 1.0, 7), rg.oracle_ref(oracle, name, 1.0, 0))
        c, (w, x, y, t) = rc.CASES[name], rc.window(name)
        with pytest.raises(hip.CmaxHipError) as e:
            be.set_window(x, y, t, c["order"], rg.point(name), w.start_ns, w.dt_ns, 0, 2 ** 62, c["batch"], c["rate"])
        assert e.value.status == _lib.ERR_INVALID_ARG


@pytest.mark.parametrize("name", ["batch1", "batch3", "batch5000", "n2", "n65", "pano130x96", "pano1000x300", "poles", "shortest4",
                                  "shortest2"])
def test_edge_shapes(hip, oracle, name):
    be = make(hip, name)
    ref = rg.oracle_ref(oracle, name, 1.0, 0)
    check(name, run(be, name), ref)
    check(name + " measure 1", run(be, name, measure=1), rg.oracle_ref(oracle, name, 1.0, 1))
    c, _ = run(be, name, want_grad=False)
    assert rel_scalar(c, ref[0]) < RTOL


@pytest.mark.parametrize("sigma", [0.0, 2.0])
@pytest.mark.parametrize("name", ["poles", "pano1000x300"])
def test_edge_shapes_other_sigmas(hip, oracle, name, sigma):
    check("%s sigma %g" % (name, sigma), run(make(hip, name), name, sigma), rg.oracle_ref(oracle, name, sigma, 0))


@pytest.mark.parametrize("name", ["n0", "n1"])
def test_nothing_to_vote(hip, name):
    c, g = run(make(hip, name), name)
    assert c == 0.0
    assert g.shape == (3 * rc.CASES[name]["K"],) and not g.any()


def test_cuts_at_batch_multiples(hip, oracle):
    pieces = rc.cuts("B", 7 * 64, 100 * 64)
    ref = rg.oracle_ref(oracle, "B")
    for det in (False, True):
        check("B cut, deterministic %d" % det, run(make(hip, "B", det), "B", pieces=pieces), ref)


def _three_paths(hip, name, deterministic):
    _, x, y, t = rc.window(name)
    be = make(hip, name, deterministic)
    store = hip.EventStore(W, H, len(x))
    store.push(x, y, t)
    out = [run(be, name, how=how, store=store) for how in ("add", "aos", "store")]
    begin(be, name)
    out.append(be.reconstruct_eval(store, 0, len(x)))
    out.append(be.reconstruct_eval(store, 0, len(x), knots=rg.point(name)))
    be.reconstruct_end()
    store.close()
    return out


def test_ingest_paths_deterministic_bit_identical(hip, oracle):
    out = _three_paths(hip, "B", True)
    for c, g in out[1:]:
        assert c == out[0][0]
        assert g.tobytes() == out[0][1].tobytes()
    check("B deterministic", out[0], rg.oracle_ref(oracle, "B"))
    again = _three_paths(hip, "B", True)  # run to run
    assert again[0][0] == out[0][0] and again[0][1].tobytes() == out[0][1].tobytes()


def test_ingest_paths_default_mode_agree(hip, oracle):
    ref = rg.oracle_ref(oracle, "B")
    for i, got in enumerate(_three_paths(hip, "B", False)):
        check("B path %d" % i, got, ref)


def test_internal_slices(hip, oracle):
    L = _lib.lib()
    _, x, y, t = rc.window("A")
    ref = rg.oracle_ref(oracle, "A")
    try:
        assert L.cmx_diag_set(_lib.DIAG_RECON_SLICE_EVENTS, 1000) == 0  # 61 slices
        for det in (False, True):
            be = make(hip, "A", det)
            store = hip.EventStore(W, H, len(x))
            store.push(x, y, t)
            for how in ("add", "store"):
                check("A in 61 slices, %s, deterministic %d" % (how, det), run(be, "A", how=how, store=store), ref)
            store.close()
    finally:
        assert L.cmx_diag_set(_lib.DIAG_RECON_SLICE_EVENTS, 0) == 0


def test_deterministic_run_to_run(hip):
    be = make(hip, "A", deterministic=True)
    a, b = run(be, "A"), run(be, "A")
    assert a[0] == b[0] and a[1].tobytes() == b[1].tobytes()


def test_a_million_knots(hip, oracle):
    """B's spline at the far end of K = 2^20 identity knots: exact zeros in front of the span, the oracle's K = 70 gradient behind"""
    c, (w, x, y, t) = rc.CASES["B"], rc.window("B")
    K = 1 << 20
    off = K - c["K"]
    knots = np.zeros((K, 4))
    knots[:, 3] = 1.0
    knots[off:] = rg.point("B")
    be = make(hip, "B")
    be.reconstruct_begin(2, knots, w.start_ns - off * w.dt_ns, w.dt_ns, c["batch"], c["rate"])
    be.reconstruct_add(x, y, t)
    con = be.reconstruct_contrast(1.0, 0, True)
    be.reconstruct_grad_add(x, y, t)
    g = be.reconstruct_grad_get()
    be.reconstruct_end()
    assert g.shape == (3 * K,)
    assert not g[:3 * off].any()
    check("B at the end of 2^20 knots", (con, g[3 * off:]), rg.oracle_ref(oracle, "B"))


def test_against_the_window_path(hip):
    """K = 10: set_window(num_fixed = 0, no map, every event old) + eval(0) on the production path is the same evaluation"""
    c, (w, x, y, t) = rc.CASES["window"], rc.window("window")
    q = rg.point("window")
    be = make(hip, "window")
    be.set_window(x, y, t, c["order"], q, w.start_ns, w.dt_ns, 0, int(t[-1]) + 1, c["batch"], c["rate"], blur_sigma=1.0)
    cw, gw = be.eval(np.zeros(be.num_params))
    store = hip.EventStore(W, H, len(x))
    store.push(x, y, t)
    begin(be, "window")
    got = be.reconstruct_eval(store, 0, len(x))
    be.reconstruct_end()
    store.close()
    assert np.abs(gw).max() > 1e-3
    check("window path", got, (cw, np.array(gw)))


def test_restart_equals_a_fresh_begin(hip):
    _, x, y, t = rc.window("B")
    q2 = rg.perturb(rc.window("B")[0].knots_true, 4242)
    for det in (True, False):
        be = make(hip, "B", det)
        fresh = run(be, "B", knots=q2)
        begin(be, "B")  # the evaluation point first, a whole evaluation there ...
        be.reconstruct_add(x, y, t)
        be.reconstruct_contrast(1.0, 0, True)
        be.reconstruct_grad_add(x, y, t)
        be.reconstruct_restart(q2)  # ... then q2 on the same buffers
        plane, n_sampled, n_inside = be.reconstruct_get(with_counts=True)
        assert n_sampled == n_inside == 0 and not plane.any()
        with pytest.raises(hip.CmaxHipError) as e:
            be.reconstruct_grad_add(x, y, t)
        assert e.value.status == _lib.ERR_STATE
        be.reconstruct_add(x, y, t)
        c = be.reconstruct_contrast(1.0, 0, True)
        be.reconstruct_grad_add(x, y, t)
        g = be.reconstruct_grad_get()
        be.reconstruct_end()
        if det:
            assert c == fresh[0] and g.tobytes() == fresh[1].tobytes()
        else:
            assert rel_scalar(c, fresh[0]) < RTOL and rel_vec(g, fresh[1]) < RTOL


def test_contrast_leaves_the_plane_and_later_adds_intact(hip):
    _, x, y, t = rc.window("B")
    be = make(hip, "B", deterministic=True)
    h = 100 * 64
    begin(be, "B")
    be.reconstruct_add(x[:h], y[:h], t[:h])
    be.reconstruct_add(x[h:], y[h:], t[h:])
    want = be.reconstruct_get(with_counts=True)
    begin(be, "B")
    be.reconstruct_add(x[:h], y[:h], t[:h])
    c1 = be.reconstruct_contrast(1.0, 0, True)
    c2 = be.reconstruct_contrast(2.0, 1, False)
    be.reconstruct_add(x[h:], y[h:], t[h:])
    got = be.reconstruct_get(with_counts=True)
    be.reconstruct_end()
    assert c1 > 0 and c2 > 0
    np.testing.assert_array_equal(got[0], want[0])
    assert got[1:] == want[1:]


def _status(hip, fn, *a, **k):
    with pytest.raises(hip.CmaxHipError) as e:
        fn(*a, **k)
    return e.value.status


def test_state_errors(hip):
    c, (w, x, y, t) = rc.CASES["window"], rc.window("window")
    store = hip.EventStore(W, H, len(x))
    store.push(x, y, t)
    grp = hip.BackendEvaluator(W, H, w.lut, c["Wp"], c["Hp"], devices=[0, 0], transport=_lib.GROUP_DIRECT)
    for be in (make(hip, "window"), grp):  # before begin, and on a group handle
        assert _status(hip, be.reconstruct_restart, rg.point("window")) == _lib.ERR_STATE
        assert _status(hip, be.reconstruct_contrast) == _lib.ERR_STATE
        assert _status(hip, be.reconstruct_grad_add, x, y, t) == _lib.ERR_STATE
        assert _status(hip, be.reconstruct_grad_add_aos, _lib.dvs_events(x, y, t)) == _lib.ERR_STATE
        assert _status(hip, be.reconstruct_grad_add_from, store, 0, len(x)) == _lib.ERR_STATE
        assert _status(hip, be.reconstruct_grad_get) == _lib.ERR_STATE
        assert _status(hip, be.reconstruct_eval, store, 0, len(x)) == _lib.ERR_STATE
    grp.close()
    be = make(hip, "window")
    begin(be, "window")
    be.reconstruct_add(x, y, t)
    assert _status(hip, be.reconstruct_grad_add, x, y, t) == _lib.ERR_STATE  # no pass is open
    assert _status(hip, be.reconstruct_grad_get) == _lib.ERR_STATE
    be.reconstruct_contrast(1.0, 0, False)  # cost-only opens none
    assert _status(hip, be.reconstruct_grad_add, x, y, t) == _lib.ERR_STATE
    be.reconstruct_contrast(1.0, 0, True)
    be.reconstruct_add(x[:200], y[:200], t[:200])  # an add in between closes it
    assert _status(hip, be.reconstruct_grad_add, x, y, t) == _lib.ERR_STATE
    assert _status(hip, be.reconstruct_grad_get) == _lib.ERR_STATE
    # one event fewer, and another cut: the counts give the caller away
    begin(be, "window")
    be.reconstruct_add(x, y, t)
    be.reconstruct_contrast(1.0, 0, True)
    be.reconstruct_grad_add(x[:-1], y[:-1], t[:-1])
    assert _status(hip, be.reconstruct_grad_get) == _lib.ERR_STATE
    be.reconstruct_contrast(1.0, 0, True)
    be.reconstruct_grad_add(x[:5001], y[:5001], t[:5001])
    be.reconstruct_grad_add(x[5001:], y[5001:], t[5001:])
    assert _status(hip, be.reconstruct_grad_get) == _lib.ERR_STATE
    be.reconstruct_contrast(1.0, 0, True)
    be.reconstruct_grad_add(x, y, t)
    g = be.reconstruct_grad_get()
    assert g.tobytes() == be.reconstruct_grad_get().tobytes() and g.any()  # may be called repeatedly
    assert _status(hip, be.reconstruct_contrast, 3.2) == _lib.ERR_INVALID_ARG  # radius 13
    be.reconstruct_end()
    store.close()


def test_a_failed_grad_add_adds_nothing(hip):
    c, (w, x, y, t) = rc.CASES["window"], rc.window("window")
    be = make(hip, "window", deterministic=True)
    want = run(be, "window")
    begin(be, "window")
    be.reconstruct_add(x, y, t)
    be.reconstruct_contrast(1.0, 0, True)
    bad_x = x.copy()
    bad_x[-2] = W
    assert _status(hip, be.reconstruct_grad_add, bad_x, y, t) == _lib.ERR_EVENT_RANGE
    only_tail = t.copy()
    only_tail[-150:] += 10_000_000_000  # the last two batches alone leave the knot support
    assert _status(hip, be.reconstruct_grad_add, x, y, only_tail) == _lib.ERR_SPLINE_RANGE
    store = hip.EventStore(W, H, len(x))
    store.push(x, y, only_tail)
    assert _status(hip, be.reconstruct_grad_add_from, store, 0, len(x)) == _lib.ERR_SPLINE_RANGE
    store.close()
    be.reconstruct_grad_add(x, y, t)
    g = be.reconstruct_grad_get()
    be.reconstruct_end()
    assert g.tobytes() == want[1].tobytes()


def test_small_panorama_has_cost_only(hip, oracle):
    """64 x 20 at sigma 3 (radius 12): Hp <= 2r + 1 -- the folded G^T cannot serve it; cost-only matches the oracle"""
    w, x, y, t = rc.window("window")
    c = rc.CASES["window"]
    q = rg.point("window")
    be = hip.BackendEvaluator(W, H, w.lut, 64, 20)
    be.reconstruct_begin(c["order"], q, w.start_ns, w.dt_ns, c["batch"], c["rate"])
    be.reconstruct_add(x, y, t)
    assert _status(hip, be.reconstruct_contrast, 3.0, 0, True) == _lib.ERR_INVALID_ARG
    con = be.reconstruct_contrast(3.0, 0, False)
    be.reconstruct_end()
    b = oracle.Backend(W, H, w.lut, 64, 20, c["order"], c["batch"], c["rate"], sigma=3.0, measure=0)
    b.set_window(x, y, t, q, w.start_ns, w.dt_ns, 0, 2 ** 62)
    ref = b.eval(np.zeros(3 * c["K"]), False)[0]
    print("64 x 20, sigma 3: %.8g against %.8g" % (con, ref))
    assert ref > 0 and rel_scalar(con, ref) < RTOL


def test_evaluation_state_untouched(hip):
    c, (w, x, y, t) = rc.CASES["window"], rc.window("window")
    be = make(hip, "window", deterministic=True)
    be.set_window(x, y, t, c["order"], w.knots_init, w.start_ns, w.dt_ns, 2, w.t_next_win_beg_ns, c["batch"], c["rate"],
                  blur_sigma=2.0)
    xa = np.random.default_rng(3).normal(0, 0.01, be.num_params)
    be.eval(xa)
    be.updateIG(200)

    def reads():
        ca, ga = be.eval(xa)
        ig, visits = be.getIG(with_visits=True)
        return (np.float64(ca).tobytes(), ga.tobytes(), ig.tobytes(), visits.tobytes(), be.get_plane(_lib.PLANE_IL_OLD).tobytes(),
                be.get_plane(_lib.PLANE_IWE).tobytes())
    reads()
    before = reads()
    store = hip.EventStore(W, H, len(x))
    store.push(x, y, t)
    begin(be, "window")
    con, g = be.reconstruct_eval(store, 0, len(x), sigma=1.0)
    be.reconstruct_end()
    store.close()
    assert con > 0 and g.any()
    assert reads() == before


def test_refinement(hip, oracle):
    c, (w, x, y, t) = rc.CASES["B"], rc.window("B")
    q0 = rg.point("B")  # (the fixed first knot carries the gauge: a common rotation of all knots hardly changes the contrast)
    be = make(hip, "B")
    store = hip.EventStore(W, H, len(x))
    store.push(x, y, t)
    knots, rep = be.reconstruct_refine(store, 0, len(x), c["order"], q0, w.start_ns, w.dt_ns, 1, event_batch_size=c["batch"],
                                       event_sample_rate=c["rate"])
    store.close()
    before, after = rg.rms_angle_deg(q0, w.knots_true), rg.rms_angle_deg(knots, w.knots_true)
    print("refinement: cost %.6g -> %.6g in %d iterations; rms orientation error %.3f deg -> %.3f deg" %
          (rep["initial_cost"], rep["final_cost"], rep["iterations"], before, after))
    assert rep["final_cost"] < rep["initial_cost"]
    ref = rg.oracle_eval(oracle, "B", x, y, t, knots, want_grad=False)[0]
    assert rel_scalar(ref, -rep["final_cost"]) < RTOL
    assert after < before


def test_example_refines_the_whole_trajectory(hip):
    import os
    import sys
    ex = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples")
    if ex not in sys.path:
        sys.path.insert(0, ex)
    import rotation_pipeline as rp
    stream = synth.event_stream(2e6, 0.5, 240, 180, 200.0, 200.0, 119.5, 89.5, omega_mean=(0.2, 1.8, 0.3),
                                omega_amp=(1.0, 0.8, 1.0), seed=77)
    res = rp.run_pipeline(stream, rp.Params(), refine_global=True)
    rep = res["refine_report"]
    assert res["refined_knots"].shape == res["traj"].knots.shape
    print("example: contrast %.6g -> %.6g" % (rep["contrast_before"], rep["contrast_after"]))
    assert rep["contrast_after"] >= rep["contrast_before"]
