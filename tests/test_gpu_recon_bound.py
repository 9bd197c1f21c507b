"""GPU: bound whole-trajectory evaluation (cmx_backend_recon_bind_from / _unbind / _eval_bound / _bound_info,
BackendEvaluator.reconstruct_bind / _unbind / _eval_bound / _bound_info, reconstruct_refine(bind=True)): the events are handed over
once, sorted by the destination tile of their vote and voted through LDS windows.

Two references.  In deterministic mode the unbound path on the SAME context (reconstruct_eval over the store): plane bytes, both
counters and the contrast must be equal, the gradient within RTOL and bitwise repeatable -- at every shape at which the sort, the
chunk table or the vote kernel can go wrong (recon_cases.py), on a panorama smaller than one LDS window, far from the sort's knots
(global path, re-sort rule), over many evaluations, through internal slices and after the store is gone.  In default mode the CPU
oracle's global_contrast_fdf (recon_grad_cases.py) at RTOL.  tests/test_recon_bound_cpu.py shows on the CPU that the small panorama
is not an empty comparison."""
import functools

import numpy as np
import pytest

import recon_cases as rc
import recon_grad_cases as rg
from cmax_slam_amd import _lib, synth
from util import RTOL, rel_scalar, rel_vec

pytestmark = pytest.mark.gpu
W, H = rc.SENSOR[:2]
SMALL = (48, 40)  # a panorama smaller than a 64 x 64 LDS window: every window hangs over the plane on all sides

DET_CASES = ["A", "B", "batch1", "batch3", "batch5000", "n2", "n65", "pano130x96", "pano1000x300", "poles", "shortest2", "shortest4"]


@functools.lru_cache(maxsize=None)
def small_window():
    """batch3's stream and spline (recon_cases.window) for the 48 x 40 panorama, and its evaluation point; read-only"""
    c = rc.CASES["batch3"]
    Wf, Hf, fx, fy, cx, cy = rc.SENSOR
    w = synth.backend_window(max(c["N"], 200), Wf, Hf, fx, fy, cx, cy, SMALL[0], SMALL[1], c["order"], c["K"], 0,
                             (c["K"] - c["order"] + 1) * rc.DT, dt_knots=rc.DT, seed=c["seed"], knot_sigma=0.02)
    x, y, t = w.x[:c["N"]].copy(), w.y[:c["N"]].copy(), w.t_ns[:c["N"]].copy()
    q = rg.perturb(w.knots_true, 1000 + c["seed"])
    for a in (x, y, t, q):
        a.setflags(write=False)
    return w, x, y, t, q


def make(hip, name, deterministic=False):
    c, w = rc.CASES[name], rc.window(name)[0]
    be = hip.BackendEvaluator(W, H, w.lut, c["Wp"], c["Hp"])
    if deterministic:
        be.set_deterministic(True)
    return be


def begin(be, name, knots=None):
    c, w = rc.CASES[name], rc.window(name)[0]
    be.reconstruct_begin(c["order"], rg.point(name) if knots is None else knots, w.start_ns, w.dt_ns, c["batch"], c["rate"])


def store_of(hip, name):
    _, x, y, t = rc.window(name)
    store = hip.EventStore(W, H, max(len(x), 1))
    if len(x):
        store.push(x, y, t)
    return store


def check(tag, got, ref):
    (c, g), (cr, gr) = got, ref
    ec, eg = rel_scalar(c, cr), (rel_vec(g, gr) if g is not None else 0.0)
    print("%s: contrast %.8g (oracle %.8g, rel %.2e), gradient rel %.2e, |g|max %.4g" % (tag, c, cr, ec, eg, np.abs(gr).max()))
    assert ec < RTOL
    assert eg < RTOL


def unbound(be, store, n, knots):
    """reconstruct_eval at `knots` and what it leaves: (contrast, gradient, plane bytes, n_sampled, n_inside)"""
    c, g = be.reconstruct_eval(store, 0, n, knots=knots)
    p, ns, ni = be.reconstruct_get(with_counts=True)
    return c, g, p.tobytes(), ns, ni


def bound(be, knots, want_grad=True):
    c, g = be.reconstruct_eval_bound(knots, want_grad=want_grad)
    p, ns, ni = be.reconstruct_get(with_counts=True)
    return c, g, p.tobytes(), ns, ni


def same(tag, got, want, grad=True):
    """deterministic mode: plane, counters and contrast equal; the gradient to summation order"""
    eg = rel_vec(got[1], want[1]) if grad and np.abs(want[1]).max() > 0 else 0.0
    print("%s: contrast %.8g / %.8g, sampled %d / %d, inside %d / %d, gradient rel %.2e" %
          (tag, got[0], want[0], got[3], want[3], got[4], want[4], eg))
    assert got[2] == want[2], "plane bytes differ"
    assert got[3:] == want[3:]
    assert got[0] == want[0]
    if grad:
        assert eg < RTOL
        if not np.abs(want[1]).max() > 0:
            assert not got[1].any()


# ---------------------------------------------------------------- 1. deterministic mode against the unbound path
@pytest.mark.parametrize("name", DET_CASES)
def test_deterministic_equals_the_unbound_path(hip, name):
    n, q = rc.CASES[name]["N"], rg.point(name)
    be = make(hip, name, deterministic=True)
    store = store_of(hip, name)
    begin(be, name)
    want = unbound(be, store, n, q)
    be.reconstruct_bind(store, 0, n)
    got = bound(be, q)
    same(name, got, want)
    again = bound(be, q)
    assert again[1].tobytes() == got[1].tobytes() and again[0] == got[0] and again[2] == got[2]
    info = be.reconstruct_bound_info()
    assert info["n_events"] == n and info["n_sampled"] == rc.sampled(n, rc.CASES[name]["batch"], rc.CASES[name]["rate"]) == got[3]
    assert info["sorts"] == 1 and info["fallback_frac"] == 0.0
    be.reconstruct_end()
    store.close()


def test_panorama_smaller_than_a_window(hip):
    w, x, y, t, q = small_window()
    c = rc.CASES["batch3"]
    be = hip.BackendEvaluator(W, H, w.lut, SMALL[0], SMALL[1])
    be.set_deterministic(True)
    store = hip.EventStore(W, H, len(x))
    store.push(x, y, t)
    be.reconstruct_begin(c["order"], q, w.start_ns, w.dt_ns, c["batch"], c["rate"])
    want = unbound(be, store, len(x), q)
    be.reconstruct_bind(store, 0, len(x))
    got = bound(be, q)
    assert want[4] > 0 and np.abs(want[1]).max() > 0  # it votes, and the gradient is not zero
    same("48 x 40", got, want)
    be.reconstruct_end()
    store.close()


def test_more_tiles_than_the_counting_sort_holds(hip):
    """4128 x 2048: 129 x 64 destination tiles, 16 513 sort keys -- above the 16 400 an LDS histogram holds, so the sort is the
    (key, index) radix sort; the smallest panorama that takes that path"""
    name = "window"
    c, (w, x, y, t) = rc.CASES[name], rc.window(name)
    q = rg.point(name)
    be = hip.BackendEvaluator(W, H, w.lut, 4128, 2048)
    be.set_deterministic(True)
    store = store_of(hip, name)
    begin(be, name)
    want = unbound(be, store, len(x), q)
    be.reconstruct_bind(store, 0, len(x))
    got = bound(be, q)
    assert want[4] > 0 and np.abs(want[1]).max() > 0
    same("4128 x 2048", got, want)
    info = be.reconstruct_bound_info()
    assert info["sorts"] == 1 and info["fallback_frac"] == 0.0
    be.reconstruct_end()
    store.close()


# ---------------------------------------------------------------- 2. default mode against the oracle
@pytest.mark.parametrize("name,sigma", [(n, 1.0) for n in rg.SIGMA1] + [(n, s) for n in rg.SIGMA02 for s in (0.0, 2.0)])
def test_default_mode_against_the_oracle(hip, oracle, name, sigma):
    n, q = rc.CASES[name]["N"], rg.point(name)
    be = make(hip, name)
    store = store_of(hip, name)
    begin(be, name)
    be.reconstruct_bind(store, 0, n)
    for measure in (0, 1):
        ref = rg.oracle_ref(oracle, name, sigma, measure)
        check("%s sigma %g measure %d" % (name, sigma, measure), be.reconstruct_eval_bound(q, sigma, measure), ref)
        c, g = be.reconstruct_eval_bound(q, sigma, measure, want_grad=False)
        assert g is None and rel_scalar(c, ref[0]) < RTOL
    be.reconstruct_end()
    store.close()


# ---------------------------------------------------------------- 3. far from the sort
def test_far_from_the_sort(hip):
    name = "A"
    n, q = rc.CASES[name]["N"], rg.point(name)
    r = np.array([[0.0, np.sin(0.5), 0.0, np.cos(0.5)]])  # 1 rad about y: 512 / (2 pi) = 81 px along the panorama, a window is 64
    far = np.ascontiguousarray(rg._quat_mul(np.repeat(r, len(q), axis=0), np.asarray(q)))
    be = make(hip, name, deterministic=True)
    store = store_of(hip, name)
    begin(be, name)
    want_q, want_far = unbound(be, store, n, q), unbound(be, store, n, far)
    assert want_far[4] > 0 and want_far[2] != want_q[2]
    be.reconstruct_bind(store, 0, n)
    same("at the sort's knots", bound(be, q), want_q)
    info = be.reconstruct_bound_info()
    assert info["sorts"] == 1 and info["fallback_frac"] == 0.0  # at the sort's own knots every voting event is in its tile's window
    same("1 rad away, old sort", bound(be, far), want_far)
    info = be.reconstruct_bound_info()
    print("fallback share one radian from the sort: %.3f" % info["fallback_frac"])
    assert info["sorts"] == 1 and info["fallback_frac"] > 0.03
    same("1 rad away, sorted again", bound(be, far), want_far)
    info = be.reconstruct_bound_info()
    assert info["sorts"] == 2 and info["fallback_frac"] == 0.0
    be.reconstruct_end()
    store.close()


# ---------------------------------------------------------------- 4. many evaluations on one binding
def test_many_evaluations_on_one_binding(hip):
    name = "B"
    n = rc.CASES[name]["N"]
    _, x, y, t = rc.window(name)
    pts = [rg.point(name), rg.perturb(rc.window(name)[0].knots_true, 4242)]
    be = make(hip, name, deterministic=True)
    store = store_of(hip, name)
    begin(be, name)
    want = [unbound(be, store, n, pts[i & 1]) for i in range(5)]
    be.reconstruct_bind(store, 0, n)
    for i in range(5):
        same("evaluation %d" % i, bound(be, pts[i & 1]), want[i])
    # other events on top, then knots = None: the plane is zeroed first, the knots stay
    be.reconstruct_add(x[:6400], y[:6400], t[:6400])
    assert be.reconstruct_get(with_counts=True)[1] > want[4][3]
    got = bound(be, None)
    same("after an add, knots kept", got, want[4])
    be.reconstruct_end()
    store.close()


# ---------------------------------------------------------------- 5. internal slices
def test_internal_slices(hip, oracle):
    L = _lib.lib()
    name = "A"
    n, q = rc.CASES[name]["N"], rg.point(name)
    ref = rg.oracle_ref(oracle, name)
    try:
        assert L.cmx_diag_set(_lib.DIAG_RECON_SLICE_EVENTS, 1000) == 0  # 61 slices of the gradient pass
        for det in (False, True):
            be = make(hip, name, det)
            store = store_of(hip, name)
            begin(be, name)
            be.reconstruct_bind(store, 0, n)
            check("A bound, 61 slices, deterministic %d" % det, be.reconstruct_eval_bound(q), ref)
            be.reconstruct_end()
            store.close()
    finally:
        assert L.cmx_diag_set(_lib.DIAG_RECON_SLICE_EVENTS, 0) == 0


# ---------------------------------------------------------------- 6. binding is a copy
def test_binding_is_a_copy(hip):
    name = "B"
    n, q = rc.CASES[name]["N"], rg.point(name)
    be = make(hip, name, deterministic=True)
    store = store_of(hip, name)
    begin(be, name)
    be.reconstruct_bind(store, 0, n)
    first = bound(be, q)
    store.close()
    again = bound(be, q)
    assert again[0] == first[0] and again[1].tobytes() == first[1].tobytes() and again[2:] == first[2:]
    assert first[4] > 0
    be.reconstruct_end()


# ---------------------------------------------------------------- 7. state and errors
def _status(hip, fn, *a, **k):
    with pytest.raises(hip.CmaxHipError) as e:
        fn(*a, **k)
    return e.value.status


def test_state_errors(hip):
    name = "window"
    c, (w, x, y, t) = rc.CASES[name], rc.window(name)
    n, q = len(x), rg.point(name)
    store = store_of(hip, name)
    grp = hip.BackendEvaluator(W, H, w.lut, c["Wp"], c["Hp"], devices=[0, 0], transport=_lib.GROUP_DIRECT)
    for be in (make(hip, name), grp):  # before begin, and on a group handle
        assert _status(hip, be.reconstruct_bind, store, 0, n) == _lib.ERR_STATE
        assert _status(hip, be.reconstruct_unbind) == _lib.ERR_STATE
        assert _status(hip, be.reconstruct_eval_bound, q) == _lib.ERR_STATE
        assert _status(hip, be.reconstruct_bound_info) == _lib.ERR_STATE
    grp.close()
    be = make(hip, name, deterministic=True)
    begin(be, name)
    assert _status(hip, be.reconstruct_eval_bound, q) == _lib.ERR_STATE  # nothing is bound
    be.reconstruct_unbind()                                              # ... which unbind does not mind
    assert be.reconstruct_bound_info() == {"n_events": 0, "n_sampled": 0, "sorts": 0, "fallback_frac": 0.0}
    be.reconstruct_bind(store, 0, n)
    want = bound(be, q)
    be.reconstruct_restart(q)  # restart keeps the binding
    same("after restart", bound(be, q), want)
    be.reconstruct_unbind()
    assert _status(hip, be.reconstruct_eval_bound, q) == _lib.ERR_STATE
    be.reconstruct_bind(store, 0, n)
    begin(be, name)  # a second begin drops it
    assert _status(hip, be.reconstruct_eval_bound, q) == _lib.ERR_STATE
    be.reconstruct_bind(store, 0, n)
    be.reconstruct_end()
    assert _status(hip, be.reconstruct_eval_bound, q) == _lib.ERR_STATE
    begin(be, name)  # ... and so did end
    assert _status(hip, be.reconstruct_eval_bound, q) == _lib.ERR_STATE
    be.reconstruct_bind(store, 0, n)
    assert _status(hip, be.reconstruct_eval_bound, q, 3.2) == _lib.ERR_INVALID_ARG  # radius 13
    same("after a refused sigma", bound(be, q), want)
    be.reconstruct_end()
    store.close()


def test_a_failed_bind_keeps_the_previous_binding(hip):
    name = "window"
    _, x, y, t = rc.window(name)
    n, q = len(x), rg.point(name)
    be = make(hip, name, deterministic=True)
    store = store_of(hip, name)
    begin(be, name)
    be.reconstruct_bind(store, 0, n)
    want = bound(be, q)
    assert _status(hip, be.reconstruct_bind, store, 0, n + 1) == _lib.ERR_INVALID_ARG  # beyond the store
    assert _status(hip, be.reconstruct_bind, store, -1, 10) == _lib.ERR_INVALID_ARG
    only_tail = t.copy()
    only_tail[-150:] += 10_000_000_000  # the last two batches alone leave the knot support
    late = hip.EventStore(W, H, n)
    late.push(x, y, only_tail)
    assert _status(hip, be.reconstruct_bind, late, 0, n) == _lib.ERR_SPLINE_RANGE
    late.close()
    assert be.reconstruct_bound_info()["n_events"] == n
    same("after three refused binds", bound(be, q), want)
    be.reconstruct_bind(store, 0, 5001)  # a second bind replaces the first
    assert be.reconstruct_bound_info()["n_events"] == 5001 and be.reconstruct_bound_info()["sorts"] == 0
    same("a prefix", bound(be, q), unbound(be, store, 5001, q))
    be.reconstruct_end()
    store.close()


@pytest.mark.parametrize("count", [0, 1])
def test_nothing_to_vote(hip, count):
    name = "n%d" % count
    q = rg.point(name)
    be = make(hip, name)
    store = store_of(hip, name)
    begin(be, name)
    be.reconstruct_bind(store, 0, count)
    assert be.reconstruct_bound_info() == {"n_events": count, "n_sampled": 0, "sorts": 0, "fallback_frac": 0.0}
    c, g = be.reconstruct_eval_bound(q)
    assert c == 0.0
    assert g.shape == (3 * rc.CASES[name]["K"],) and not g.any()
    assert be.reconstruct_get(with_counts=True)[1:] == (0, 0)
    be.reconstruct_end()
    store.close()


# ---------------------------------------------------------------- 8. window state untouched
def test_window_state_untouched(hip):
    name = "window"
    c, (w, x, y, t) = rc.CASES[name], rc.window(name)
    be = make(hip, name, deterministic=True)
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

    def rebins():
        return be.stats()["rebins"]
    sorts_before = rebins()
    assert sorts_before >= 1
    store = store_of(hip, name)
    begin(be, name)
    be.reconstruct_bind(store, 0, len(x))
    con, g = be.reconstruct_eval_bound(rg.point(name), sigma=1.0)
    assert be.reconstruct_bound_info()["sorts"] == 1
    be.reconstruct_end()
    store.close()
    assert con > 0 and g.any()
    assert rebins() == sorts_before
    assert reads() == before
    assert rebins() == sorts_before  # (the window's own sort is still the one it evaluates with)


# ---------------------------------------------------------------- 9. refinement
def _refine(hip, det, bind):
    name = "B"
    c, (w, x, y, t) = rc.CASES[name], rc.window(name)
    be = make(hip, name, det)
    store = store_of(hip, name)
    knots, rep = be.reconstruct_refine(store, 0, len(x), c["order"], rg.point(name), w.start_ns, w.dt_ns, 1, event_batch_size=c["batch"],
                                       event_sample_rate=c["rate"], bind=bind)
    store.close()
    return knots, rep


def test_refinement_bound(hip, oracle):
    """test_refinement's three assertions for bind=True, in default and in deterministic mode.  In deterministic mode the knots are
    compared BYTEWISE with those of bind=False (not the final contrasts at RTOL): the gather pass over the bound copy keeps the
    unbound pass's slices, runs and order of sums, so the two gradients agree in every bit and the two solves take the same steps."""
    name = "B"
    _, x, y, t = rc.window(name)
    w = rc.window(name)[0]
    q0 = rg.point(name)
    knots, rep = _refine(hip, False, True)
    before, after = rg.rms_angle_deg(q0, w.knots_true), rg.rms_angle_deg(knots, w.knots_true)
    print("bound refinement: cost %.6g -> %.6g in %d iterations; rms orientation error %.3f deg -> %.3f deg" %
          (rep["initial_cost"], rep["final_cost"], rep["iterations"], before, after))
    assert rep["final_cost"] < rep["initial_cost"]
    ref = rg.oracle_eval(oracle, name, x, y, t, knots, want_grad=False)[0]
    assert rel_scalar(ref, -rep["final_cost"]) < RTOL
    assert after < before
    kb, rb = _refine(hip, True, True)
    ku, ru = _refine(hip, True, False)
    print("deterministic mode, bind=True against bind=False: max |dq| %.2e; final cost %.10g / %.10g" %
          (np.abs(kb - ku).max(), rb["final_cost"], ru["final_cost"]))
    assert kb.tobytes() == ku.tobytes()
    assert rb["final_cost"] == ru["final_cost"]
    assert rb["final_cost"] < rb["initial_cost"]
    assert rel_scalar(rg.oracle_eval(oracle, name, x, y, t, kb, want_grad=False)[0], -rb["final_cost"]) < RTOL
    assert rg.rms_angle_deg(kb, w.knots_true) < before
