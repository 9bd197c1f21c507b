"""GPU: the frozen head of a bound whole-trajectory evaluation and the native solve over it (cmx_backend_recon_freeze_head /
_frozen_info / _solve; BackendEvaluator.reconstruct_freeze_head / _frozen_info / _solve).

References.  In deterministic mode the SAME binding without a frozen head: plane bytes, both counters and the contrast must be equal
(fixed-point adds commute, the moment rows are ordered), the free gradient entries within RTOL of the unfrozen gradient's max-norm
(the gather's runs start at the first active batch, so only the order of sums differs; bitwise when no batch is frozen), the fixed
entries exactly zero.  In default mode the CPU oracle's global_contrast_fdf with num_fixed (recon_grad_cases.oracle_eval) at RTOL.
For the solve: BackendEvaluator.reconstruct_refine(bind=True), the same FR-CG machine driven from Python -- in deterministic mode
the native call must return its knots byte for byte.  tests/test_recon_solve_cpu.py checks the prefix rule on the CPU."""
import numpy as np
import pytest

import recon_cases as rc
import recon_grad_cases as rg
from cmax_slam_amd import _lib
from test_gpu_recon_bound import SMALL, W, H, begin, bound, make, small_window, store_of
from util import RTOL, rel_scalar, rel_vec

pytestmark = pytest.mark.gpu

DET_CASES = ["A", "B", "batch1", "batch5000", "shortest2", "shortest4", "n65", "poles"]


def fixed_counts(order, K):
    """num_fixed at order - 1 (nothing frozen), in mid-trajectory and at K - 1, each once"""
    return sorted({order - 1, max(K // 2, 1), K - 1})


def frozen_batches_of(name, nf, n=None):
    """the prefix rule, restated: batch pose times from the stream (midpoint of first and last event), segment, s + order - 1 < nf"""
    c, (w, x, y, t) = rc.CASES[name], rc.window(name)
    t = t[:n] if n is not None else t
    n = len(t)
    if n < 2:
        return 0, 0
    B = c["batch"]
    nb = (n - 1 + B - 1) // B
    count = 0
    for b in range(nb):
        lo, hi = b * B, (b * B + B if n - b * B > B else n)
        tb = int(t[lo]) + (int(t[hi - 1]) - int(t[lo])) // 2  # (to a nanosecond of the library's rounding: no case sits on a boundary)
        s = min((tb - w.start_ns) // w.dt_ns, c["K"] - c["order"])
        if s + c["order"] - 1 < nf:
            count += 1
        else:
            break
    return count, nb


def check_frozen(tag, be, q, want, nf, expect_batches=None):
    """one frozen evaluation at q against `want`, the unfrozen evaluation of the same binding at q (deterministic mode)"""
    be.reconstruct_freeze_head(nf)
    info = be.reconstruct_frozen_info()
    got = bound(be, q)
    g, gw = got[1], want[1]
    scale = np.abs(gw).max()
    eg = np.abs(g[3 * nf:] - gw[3 * nf:]).max() / scale if scale > 0 else 0.0
    print("%s num_fixed %d: %d batches / %d events frozen; contrast %.8g / %.8g, inside %d / %d, free gradient rel %.2e" %
          (tag, nf, info["frozen_batches"], info["frozen_sampled"], got[0], want[0], got[4], want[4], eg))
    assert info["num_fixed"] == nf
    if expect_batches is not None:
        assert info["frozen_batches"] == expect_batches
    assert got[2] == want[2], "plane bytes differ"
    assert got[3:] == want[3:]
    assert got[0] == want[0]
    assert not g[:3 * nf].any()
    assert eg < RTOL
    if scale == 0:
        assert not g.any()
    if info["frozen_batches"] == 0:
        assert g[3 * nf:].tobytes() == gw[3 * nf:].tobytes()
    again = be.reconstruct_grad_get()  # grad_get repeats it, its consistency test holds for base plus active
    assert again.tobytes() == g.tobytes()
    assert be.reconstruct_frozen_info() == info  # eval_bound keeps the frozen head
    return info, got


# ---------------------------------------------------------------- 1. frozen equals unfrozen, deterministic mode
@pytest.mark.parametrize("name", DET_CASES)
def test_frozen_equals_unfrozen(hip, name):
    c = rc.CASES[name]
    n, q = c["N"], rg.point(name)
    be = make(hip, name, deterministic=True)
    store = store_of(hip, name)
    begin(be, name)
    be.reconstruct_bind(store, 0, n)
    want = bound(be, q)
    assert be.reconstruct_frozen_info() == {"num_fixed": 0, "frozen_batches": 0, "frozen_sampled": 0}
    some = 0
    for nf in fixed_counts(c["order"], c["K"]):
        fb, nb = frozen_batches_of(name, nf)
        info, _ = check_frozen(name, be, q, want, nf, fb)
        per_batch = (c["batch"] + c["rate"] - 1) // c["rate"]  # (whole batches in front of an active one; all of them: the stream's count)
        assert info["frozen_sampled"] == (fb * per_batch if fb < nb else rc.sampled(n, c["batch"], c["rate"]))
        some += fb
    if name not in ("shortest2", "shortest4", "n65"):  # (K = order, or one batch at the far end: nothing can freeze there)
        assert some > 0
    be.reconstruct_freeze_head(0)  # removed: the unfrozen evaluation again, bit for bit, gradient included
    assert be.reconstruct_frozen_info()["num_fixed"] == 0
    back = bound(be, q)
    assert back[0] == want[0] and back[1].tobytes() == want[1].tobytes() and back[2:] == want[2:]
    be.reconstruct_end()
    store.close()


def test_frozen_on_a_panorama_smaller_than_a_window(hip):
    w, x, y, t, q = small_window()
    c = rc.CASES["batch3"]
    be = hip.BackendEvaluator(W, H, w.lut, SMALL[0], SMALL[1])
    be.set_deterministic(True)
    store = hip.EventStore(W, H, len(x))
    store.push(x, y, t)
    be.reconstruct_begin(c["order"], q, w.start_ns, w.dt_ns, c["batch"], c["rate"])
    be.reconstruct_bind(store, 0, len(x))
    want = bound(be, q)
    assert want[4] > 0 and np.abs(want[1]).max() > 0
    frozen = 0
    for nf in fixed_counts(c["order"], c["K"]):
        frozen += check_frozen("48 x 40", be, q, want, nf)[0]["frozen_batches"]
    assert frozen > 0
    be.reconstruct_end()
    store.close()


# ---------------------------------------------------------------- 2. default mode against the oracle
_oracle_refs = {}


def oracle_fixed(oracle, name, sigma, measure, nf):
    key = (name, sigma, measure, nf)
    if key not in _oracle_refs:
        _, x, y, t = rc.window(name)
        cr, gr = rg.oracle_eval(oracle, name, x, y, t, rg.point(name), sigma, measure, num_fixed=nf)
        _oracle_refs[key] = (cr, np.array(gr, copy=True))
    return _oracle_refs[key]


@pytest.mark.parametrize("name,sigma", [(n, 1.0) for n in rg.SIGMA1] + [(n, 2.0) for n in rg.SIGMA02])
def test_default_mode_against_the_oracle(hip, oracle, name, sigma):
    c = rc.CASES[name]
    n, q, K = c["N"], rg.point(name), c["K"]
    nf = max(K // 2, 1)
    be = make(hip, name)
    store = store_of(hip, name)
    begin(be, name)
    be.reconstruct_bind(store, 0, n)
    be.reconstruct_freeze_head(nf)
    for measure in (0, 1):
        cr, gr = oracle_fixed(oracle, name, sigma, measure, nf)
        assert gr.shape == (3 * (K - nf),)
        con, g = be.reconstruct_eval_bound(q, sigma, measure)
        ec, eg = rel_scalar(con, cr), rel_vec(g[3 * nf:], gr)
        print("%s sigma %g measure %d num_fixed %d (%d batches frozen): contrast %.8g (oracle %.8g, rel %.2e), gradient rel %.2e" %
              (name, sigma, measure, nf, be.reconstruct_frozen_info()["frozen_batches"], con, cr, ec, eg))
        assert ec < RTOL and eg < RTOL
        assert not g[:3 * nf].any()
        con2, g2 = be.reconstruct_eval_bound(q, sigma, measure, want_grad=False)
        assert g2 is None and rel_scalar(con2, cr) < RTOL
    be.reconstruct_end()
    store.close()


# ---------------------------------------------------------------- 3. all frozen
def test_all_frozen(hip):
    """the events end before the free knots' support: half of A's stream under num_fixed = K - 1"""
    name = "A"
    c = rc.CASES[name]
    n, q, nf = c["N"] // 2, rg.point(name), c["K"] - 1
    fb, nb = frozen_batches_of(name, nf, n)
    assert fb == nb > 0
    be = make(hip, name, deterministic=True)
    store = store_of(hip, name)
    begin(be, name)
    be.reconstruct_bind(store, 0, n)
    want_cost = be.reconstruct_eval_bound(q, want_grad=False)[0]  # (the cost-only image pass sums other rows than the adjoint one)
    want = bound(be, q)
    assert want[4] > 0
    info, got = check_frozen("all frozen", be, q, want, nf, nb)
    assert info["frozen_sampled"] == want[3] == rc.sampled(n, c["batch"], c["rate"])
    assert not got[1][3 * nf:].any() and not want[1][3 * nf:].any()
    con, g = be.reconstruct_eval_bound(q, want_grad=False)
    assert con == want_cost and g is None
    be.reconstruct_end()
    store.close()


# ---------------------------------------------------------------- 4. far from the sort
def test_far_from_the_sort(hip):
    name = "A"
    c = rc.CASES[name]
    n, q, nf = c["N"], rg.point(name), c["K"] // 2
    r = np.array([[0.0, np.sin(0.5), 0.0, np.cos(0.5)]])  # 1 rad about y: 81 px along the panorama, a window is 64
    far = np.array(q, copy=True)
    far[nf:] = rg._quat_mul(np.repeat(r, len(q) - nf, axis=0), np.asarray(q)[nf:])  # the free knots alone
    far = np.ascontiguousarray(far)
    be = make(hip, name, deterministic=True)
    store = store_of(hip, name)
    begin(be, name)
    be.reconstruct_bind(store, 0, n)
    want_q, want_far = bound(be, q), bound(be, far)
    assert want_far[4] > 0 and want_far[2] != want_q[2]
    be.reconstruct_eval_bound(q, want_grad=False)  # (the knots the head is frozen at)
    info, _ = check_frozen("at the sort's knots", be, q, want_q, nf)
    assert info["frozen_batches"] > 0
    sorts = be.reconstruct_bound_info()["sorts"]
    assert be.reconstruct_bound_info()["fallback_frac"] == 0.0
    got = bound(be, far)
    bi = be.reconstruct_bound_info()
    print("fallback share of the active votes one radian from the sort: %.3f" % bi["fallback_frac"])
    assert got[2] == want_far[2] and got[3:] == want_far[3:] and got[0] == want_far[0]
    assert bi["sorts"] == sorts and bi["fallback_frac"] > 0.03
    got = bound(be, far)
    bi = be.reconstruct_bound_info()
    assert got[2] == want_far[2] and got[3:] == want_far[3:] and got[0] == want_far[0]
    assert rel_vec(got[1][3 * nf:], want_far[1][3 * nf:]) < RTOL
    assert bi["sorts"] == sorts + 1 and bi["fallback_frac"] == 0.0
    assert be.reconstruct_frozen_info() == info
    be.reconstruct_end()
    store.close()


# ---------------------------------------------------------------- 5. the fixed prefix is enforced; what drops a frozen head
def _status(hip, fn, *a, **k):
    with pytest.raises(hip.CmaxHipError) as e:
        fn(*a, **k)
    return e.value.status


def test_fixed_prefix_is_enforced(hip):
    name = "B"
    c = rc.CASES[name]
    n, q, nf = c["N"], rg.point(name), c["K"] // 2
    none = {"num_fixed": 0, "frozen_batches": 0, "frozen_sampled": 0}
    be = make(hip, name, deterministic=True)
    store = store_of(hip, name)
    begin(be, name)
    assert _status(hip, be.reconstruct_freeze_head, nf) == _lib.ERR_STATE  # nothing is bound
    assert be.reconstruct_frozen_info() == none
    be.reconstruct_bind(store, 0, n)
    assert _status(hip, be.reconstruct_freeze_head, -1) == _lib.ERR_INVALID_ARG
    assert _status(hip, be.reconstruct_freeze_head, c["K"]) == _lib.ERR_INVALID_ARG
    be.reconstruct_freeze_head(nf)
    before = bound(be, q)
    info = be.reconstruct_frozen_info()
    assert info["frozen_batches"] > 0
    bad = np.array(q, copy=True)
    bad[nf - 1] = rg.perturb(q[nf - 1:nf], 99)[0]  # the last fixed knot, changed
    assert _status(hip, be.reconstruct_eval_bound, bad) == _lib.ERR_INVALID_ARG
    assert be.reconstruct_frozen_info() == info
    p, ns, ni = be.reconstruct_get(with_counts=True)  # nothing changed: the plane is still the last evaluation's
    assert p.tobytes() == before[2] and (ns, ni) == before[3:]
    after = bound(be, q)
    assert after[0] == before[0] and after[1].tobytes() == before[1].tobytes() and after[2:] == before[2:]
    free_moved = np.array(q, copy=True)
    free_moved[nf:] = rg.perturb(q[nf:], 98)
    be.reconstruct_eval_bound(np.ascontiguousarray(free_moved))  # free knots may move
    be.reconstruct_restart(q)  # restart drops the frozen head
    assert be.reconstruct_frozen_info() == none
    be.reconstruct_eval_bound(bad)  # ... so any knots are fine again
    be.reconstruct_eval_bound(q, want_grad=False)
    be.reconstruct_freeze_head(nf)
    assert be.reconstruct_frozen_info() == info
    be.reconstruct_bind(store, 0, n)  # and so does bind_from
    assert be.reconstruct_frozen_info() == none
    be.reconstruct_freeze_head(nf)
    be.reconstruct_unbind()
    assert be.reconstruct_frozen_info() == none
    be.reconstruct_end()
    store.close()


# ---------------------------------------------------------------- 6. window state untouched
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
    be.reconstruct_freeze_head(c["K"] // 2)
    con, g = be.reconstruct_eval_bound(rg.point(name), sigma=1.0)
    knots, rep = be.reconstruct_solve(rg.point(name), c["K"] // 2, freeze_head=True, max_iterations=3)
    assert be.reconstruct_frozen_info()["num_fixed"] == c["K"] // 2
    be.reconstruct_end()
    store.close()
    assert con > 0 and g.any() and rep["n_df"] >= 1
    assert rebins() == sorts_before
    assert reads() == before
    assert rebins() == sorts_before  # (the window's own sort is still the one it evaluates with)


# ---------------------------------------------------------------- 7. the native solve equals the Python route
def _case():
    name = "B"
    return name, rc.CASES[name], rc.window(name)


def _refine_python(hip, det):
    name, c, (w, x, y, t) = _case()
    be = make(hip, name, det)
    store = store_of(hip, name)
    knots, rep = be.reconstruct_refine(store, 0, len(x), c["order"], rg.point(name), w.start_ns, w.dt_ns, 1, event_batch_size=c["batch"],
                                       event_sample_rate=c["rate"], bind=True)
    store.close()
    return knots, rep


def _solve_native(hip, det, num_fixed=1, freeze_head=False):
    """begin + bind + reconstruct_solve on B; the evaluator is returned open, at the refined knots' evaluation"""
    name, c, (w, x, y, t) = _case()
    be = make(hip, name, det)
    store = store_of(hip, name)
    begin(be, name)
    be.reconstruct_bind(store, 0, len(x))
    knots, rep = be.reconstruct_solve(rg.point(name), num_fixed, freeze_head=freeze_head)
    store.close()
    return be, knots, rep


def test_native_solve_equals_the_python_route(hip, oracle):
    name, c, (w, x, y, t) = _case()
    q0 = rg.point(name)
    kp, rp = _refine_python(hip, True)
    be, kn, rn = _solve_native(hip, True)
    print("deterministic mode, native against Python: max |dq| %.2e; %d / %d iterations, n_f %d / %d, n_df %d / %d, cost %.10g / %.10g" %
          (np.abs(kn - kp).max(), rn["iterations"], rp["iterations"], rn["n_f"], rp["n_f"], rn["n_df"], rp["n_df"], rn["final_cost"],
           rp["final_cost"]))
    assert kn.tobytes() == kp.tobytes()
    assert rn == rp  # iterations, status, evaluation counts, initial and final cost
    assert rn["iterations"] >= 1 and rn["final_cost"] < rn["initial_cost"]
    # after the call the reconstruction holds the refined knots' evaluation
    plane, ns, ni = be.reconstruct_get(with_counts=True)
    evals, waits = be.reconstruct_solve_counts()
    print("native solve: %d evaluations, %d host waits inside them" % (evals, waits))
    assert rn["n_f"] + rn["n_df"] <= evals <= rn["n_f"] + rn["n_df"] + 1
    want = bound(be, kn)
    assert plane.tobytes() == want[2] and (ns, ni) == want[3:]
    # (the accepted cost of a line search is a cost-only evaluation's: compared with one, bit for bit)
    assert -rn["final_cost"] == be.reconstruct_eval_bound(kn, want_grad=False)[0]
    be.reconstruct_end()
    # default mode: test_refinement_bound's three assertions
    be, knots, rep = _solve_native(hip, False)
    before, after = rg.rms_angle_deg(q0, w.knots_true), rg.rms_angle_deg(knots, w.knots_true)
    print("native refinement: cost %.6g -> %.6g in %d iterations; rms orientation error %.3f deg -> %.3f deg" %
          (rep["initial_cost"], rep["final_cost"], rep["iterations"], before, after))
    assert rep["final_cost"] < rep["initial_cost"]
    ref = rg.oracle_eval(oracle, name, x, y, t, knots, want_grad=False)[0]
    assert rel_scalar(ref, -rep["final_cost"]) < RTOL
    assert after < before
    assert rep["status"] in (0, -2, 27) and rep["n_df"] >= 1 and rep["iterations"] >= 1
    be.reconstruct_end()


# ---------------------------------------------------------------- 8. solve with a frozen head
def test_solve_with_a_frozen_head(hip):
    name, c, (w, x, y, t) = _case()
    q0, nf = rg.point(name), c["K"] // 2
    be, knots, rep = _solve_native(hip, True, nf, freeze_head=True)
    info = be.reconstruct_frozen_info()
    print("frozen solve: num_fixed %d, %d batches / %d events frozen; cost %.8g -> %.8g in %d iterations (status %d)" %
          (nf, info["frozen_batches"], info["frozen_sampled"], rep["initial_cost"], rep["final_cost"], rep["iterations"], rep["status"]))
    assert info["num_fixed"] == nf and info["frozen_batches"] > 0  # the frozen head is left in place
    assert rep["status"] in (0, 27) and rep["iterations"] >= 1  # it converges: not the iteration limit
    assert knots[:nf].tobytes() == np.asarray(q0)[:nf].tobytes()
    assert knots[nf:].tobytes() != np.asarray(q0)[nf:].tobytes()
    assert -rep["final_cost"] >= -rep["initial_cost"]
    plane = be.reconstruct_get()
    con_frozen = be.reconstruct_eval_bound(knots, want_grad=False)[0]
    assert con_frozen == -rep["final_cost"] and be.reconstruct_get().tobytes() == plane.tobytes()
    be.reconstruct_freeze_head(0)
    con = be.reconstruct_eval_bound(knots, want_grad=False)[0]
    print("refined contrast, frozen %.10g / unfrozen %.10g" % (con_frozen, con))
    assert rel_scalar(con_frozen, con) < RTOL
    be.reconstruct_end()


# ---------------------------------------------------------------- 9. solve errors
def test_solve_errors(hip):
    name, c, (w, x, y, t) = _case()
    q = rg.point(name)
    be = make(hip, name, deterministic=True)
    store = store_of(hip, name)
    begin(be, name)
    assert _status(hip, be.reconstruct_solve, q, 1) == _lib.ERR_STATE  # no binding
    be.reconstruct_bind(store, 0, len(x))
    before = bound(be, q)

    def unchanged(tag):
        p, ns, ni = be.reconstruct_get(with_counts=True)
        assert p.tobytes() == before[2] and (ns, ni) == before[3:], tag  # nothing changed ...
        again = bound(be, q)
        assert again[0] == before[0] and again[1].tobytes() == before[1].tobytes() and again[2:] == before[2:], tag  # ... nor evaluates otherwise
        assert be.reconstruct_bound_info()["sorts"] == 1

    assert _status(hip, be.reconstruct_solve, q, c["K"]) == _lib.ERR_INVALID_ARG
    unchanged("num_fixed = K")
    assert _status(hip, be.reconstruct_solve, q, -1) == _lib.ERR_INVALID_ARG
    unchanged("num_fixed = -1")
    assert _status(hip, be.reconstruct_solve, q, 1, step_size=float("nan")) == _lib.ERR_INVALID_ARG
    unchanged("NaN step size")
    assert _status(hip, be.reconstruct_solve, q, 1, freeze_head=True, tol=float("inf")) == _lib.ERR_INVALID_ARG
    unchanged("infinite tol")
    assert _status(hip, be.reconstruct_solve, q, 1, 3.2) == _lib.ERR_INVALID_ARG  # radius 13
    unchanged("sigma beyond the blur's radius")
    assert be.reconstruct_frozen_info()["num_fixed"] == 0
    be.reconstruct_end()
    store.close()
