"""-m gpu: what a context keeps BETWEEN calls, on sparse scenes.

Almost every other test hands a fresh context one dense packet and compares a handful of evaluations.  On a dense scene every
tile is active, so whatever an earlier call left in the ping-pong partner is cleared by the next image pass whether the host's
bookkeeping (accum_clean / alt_clean, votes_bin_id, last_fallback_flags, fallback_pending, force_rebin, jt_valid, x_valid, the warm
end of a device-driven solve) is right or not.  Here the scenes are sparse (tests/seq_cases.py): the fused splat clears the partner
only under the tiles whose image pass runs, so votes left in an inactive tile come back as a wrong contrast two evaluations
later.  The oracle is stateless in everything the front end returns: whatever the context did before, call k must return what the
oracle returns for call k's arguments, within util.RTOL.

Directed sequences (each asserts from stats() that it ran the path it is about) and seeded walks over the whole alphabet of
calls; production path, default options unless the list switches them.  In deterministic mode every contrast, gradient and plane
of a walk must be bit-identical to what a fresh deterministic context returns for the same call alone.
"""
import numpy as np
import pytest

import display_ref as dr
import seq_cases as sc
from cmax_slam_amd import _lib
from util import RTOL, rel_img, rel_scalar, rel_vec

pytestmark = pytest.mark.gpu

OM0, EPS = sc.OMEGA0, sc.EPS


# ------------------------------------------------------------------------------------------------- front end: plumbing
def _set_packet(fe, name):
    p = sc.packet(name)
    fe.set_packet(p.x, p.y, p.t_ns, p.t_ref_ns, p.fx, p.fy, p.cx, p.cy, p.batch, p.sigma, _lib.VARIANCE)


def _fe(hip, name, deterministic=False):
    p = sc.packet(name)
    fe = hip.FrontendEvaluator(p.W, p.H, p.lut)
    if deterministic:
        fe.set_deterministic()
    _set_packet(fe, name)
    return fe


def _check_eval(fe, name, x, msg, want_grad=True):
    c_ref, g_ref = sc.fe_oracle(name).eval(x)
    c, g = fe.eval(x, want_grad)
    print("%s: contrast %.9g (oracle %.9g, rel %.2e)%s" % (msg, c, c_ref, rel_scalar(c, c_ref),
                                                            " gradient rel %.2e" % rel_vec(g, g_ref) if want_grad else ""))
    assert rel_scalar(c, c_ref) < RTOL, (msg, c, c_ref)
    if want_grad:
        assert rel_vec(g, g_ref) < RTOL, (msg, g, g_ref)


def _check_image(fe, name, x, blur, deriv, msg):
    ref = sc.fe_oracle(name)
    if deriv:
        img, d = fe.computeImageOfWarpedEvents(x, want_deriv=True, blur=blur)
        img_ref, d_ref = ref.iwe(x, deriv=True, blur=blur)
        for k in range(3):
            assert rel_img(d[..., k], d_ref[..., k]) < RTOL, (msg, k)
    else:
        img, img_ref = fe.computeImageOfWarpedEvents(x, blur=blur), ref.iwe(x, blur=blur)
    assert rel_img(img, img_ref) < RTOL, msg     # the bound of test_gpu_lds_splat.py::test_frontend_lds_iwe_image


def _check_display(fe, name, x, msg):
    ref = sc.fe_oracle(name)
    out = fe.publishEventImage(x)
    # the planes are voted with fp32 atomics: levels as tests/test_gpu_display.py::test_frontend_pair_atomic_planes compares them
    try:
        dr.assert_within_one(out, dr.local_pair_levels(ref.iwe(np.zeros(3), blur=False), ref.iwe(x, blur=False)))
    except AssertionError as e:
        raise AssertionError("%s: %s" % (msg, e)) from e


def _three_near(fe, name, st, msg, strict=True):
    """eval(OM0 + k EPS), k = 1..3, each against the oracle; the second one cost-only.  A fused evaluation takes its moments from
    the passes of the ACTIVE tiles alone (a tile with nbr_expected == 0 returns at once), so votes left in an inactive tile are
    invisible to it -- a sequence of gradient evaluations alone passes over a dirty plane.  The next evaluation whose image pass
    covers the whole plane (cost-only, eval_many, an image read-back) reads them; it votes into the plane of the evaluation
    before last.  strict: no sort in between, one fused evaluation per plain gradient evaluation, none repeated."""
    for k in (1, 2, 3):
        _check_eval(fe, name, OM0 + k * EPS, "%s, near evaluation %d" % (msg, k), want_grad=k != 2)
    end = fe.stats()
    print(msg, "before:", st, "after:", end)
    assert end["fused_evals"] >= st["fused_evals"] + 2, (msg, st, end)
    if strict:
        assert end["rebins"] == st["rebins"], (msg, st, end)
        assert end["fused_evals"] == st["fused_evals"] + 2 and end["fused_redos"] == st["fused_redos"], (msg, st, end)
    return end


# ------------------------------------------------------------------------------------------------- directed sequences
LISTS = {
    "far": lambda n: [sc.far_point(n, OM0)],
    "near_far": lambda n: [OM0 + 0.5 * EPS, sc.far_point(n, OM0)],
    "reach_far": lambda n: [sc.reach_point(n, OM0), sc.far_point(n, OM0)],   # (packet C: one within the reach, one beyond it)
    "far_reach": lambda n: [sc.far_point(n, OM0), sc.reach_point(n, OM0)],   # the planes hold the LAST candidate's votes
}


@pytest.mark.parametrize("name,which,grads", [("A", "far", True), ("A", "near_far", True), ("A", "far", False), ("B", "far", True),
                                              ("B", "near_far", False), ("C", "reach_far", True), ("C", "far_reach", True)])
def test_far_list_then_near_evaluations(hip, oracle, name, which, grads):
    """eval(w0); eval_many(list ending far away); eval(w0 + e), eval(w0 + 2e, cost only), eval(w0 + 3e).  The list's last
    candidate votes beyond kFuseReach with 3 % or fewer votes outside their windows: no new sort.  eval_many used to refresh the
    fallback share only, not the reach flags, which stayed those of eval(w0) (none raised): the fused evaluation at w0 + e took the
    partner as covered by its tiles' passes, cleared only the active tiles and called it clean, and the evaluation at w0 + 2e
    voted into a plane that still held the far votes.  far_reach: the flags are those of the LAST candidate, not of any."""
    fe = _fe(hip, name)
    ref = sc.fe_oracle(name)
    msg = "packet %s, list %s, %s" % (name, which, "gradients" if grads else "cost only")
    _check_eval(fe, name, OM0, msg + ", first evaluation")
    st = fe.stats()
    assert st["rebins"] == 1 and st["fused_evals"] == 1 and st["fallback_frac"] == 0, st
    xs = np.array(LISTS[which](name))
    cs, gs = fe.eval_many(xs, grads)
    for i, x in enumerate(xs):
        c_ref, g_ref = ref.eval(x)
        assert rel_scalar(cs[i], c_ref) < RTOL, (msg, i, cs[i], c_ref)
        if grads:
            assert rel_vec(gs[i], g_ref) < RTOL, (msg, i, gs[i], g_ref)
    st = fe.stats()
    assert 0 < st["fallback_frac"] <= 0.03 and st["rebins"] == 1, (msg, st)
    assert st["fallback_frac"] == pytest.approx(sc.fallback_share(sc.packet(name), OM0, xs[-1]), abs=2e-3)
    _three_near(fe, name, st, msg)


@pytest.mark.parametrize("name", ["A", "B"])
@pytest.mark.parametrize("call", ["image", "image_blurred", "display"])
def test_far_image_then_near_evaluations(hip, oracle, name, call):
    """The same with an image read-back or a render at the far point in place of the list.  The blurred read-back runs a finalize:
    its fallback share and reach flags are the call's own (asserted), and the near evaluations run without a new sort.  The
    unblurred read-back and the render end without one.  sync_and_collect then leaves kFuseUnsafe, so that nothing is assumed
    about where those votes went; no sequence here depends on it, because such a call also leaves the partner marked dirty and
    its fallback word on the device -- the next evaluation clears its plane whole, reports that word as its own and repeats
    itself after a new sort (slower, not wrong; hence strict=False).  That branch is right by construction, not by a test that
    failed without it."""
    fe = _fe(hip, name)
    msg = "packet %s, %s" % (name, call)
    _check_eval(fe, name, OM0, msg + ", first evaluation")
    far = sc.far_point(name, OM0)
    if call == "display":
        _check_display(fe, name, far, msg)
    else:
        _check_image(fe, name, far, call == "image_blurred", False, msg)
    st = fe.stats()
    assert st["rebins"] == 1 and st["fused_evals"] == 1, (msg, st)
    if call == "image_blurred":
        assert 0 < st["fallback_frac"] <= 0.03, (msg, st)
    _three_near(fe, name, st, msg, strict=call == "image_blurred")


@pytest.mark.parametrize("name", ["A", "B"])
def test_far_evaluation_repeats_itself(hip, oracle, name):
    """eval(w0); eval(far): the fused evaluation reports votes beyond the reach and repeats itself after a sort at its own point
    (fused_redos + 1); then the near points, from which the far group is beyond the reach of THAT sort."""
    fe = _fe(hip, name)
    msg = "packet %s" % name
    _check_eval(fe, name, OM0, msg + ", first evaluation")
    st = fe.stats()
    _check_eval(fe, name, sc.far_point(name, OM0), msg + ", far evaluation")
    end = fe.stats()
    assert end["fused_redos"] == st["fused_redos"] + 1 and end["rebins"] == st["rebins"] + 1, (st, end)
    _three_near(fe, name, end, msg, strict=False)   # (the first of them repeats itself as well)


def test_solve_that_sorts_again_then_evaluations_then_a_second_solve(hip, oracle):
    """A solve from a far point: its first fused slot votes beyond the reach of the sort made at w0, so the host takes over and
    sorts again at the start (chain_takeovers and rebins grow during the solve).  Then near evaluations, then a second,
    device-driven solve from the first one's estimate, which must reach the final cost of a host-driven solve of a fresh context.  final_cost is the machine's f at
    the returned x (cmx_solver.cpp Machine::report: x = s.x, final_cost = s.f, the pair the FR-CG iteration accepted together), so
    its negative is also the oracle's contrast there."""
    name = "A"
    ref = sc.fe_oracle(name)
    fe = _fe(hip, name)
    _check_eval(fe, name, OM0, "first evaluation")
    st = fe.stats()
    start = sc.far_point(name, OM0)
    x1, rep1 = fe.setupProblemAndOptimize(start)
    end = fe.stats()
    print("first solve:", x1, rep1, end)
    assert end["rebins"] > st["rebins"] and end["chain_solves"] == st["chain_solves"] + 1, (st, end)
    assert end["chain_takeovers"] == st["chain_takeovers"] + 1, (st, end)
    assert rel_scalar(-rep1["initial_cost"], ref.eval(start, False)[0]) < RTOL
    assert rel_scalar(-rep1["final_cost"], ref.eval(x1, False)[0]) < RTOL, (x1, rep1)
    assert rep1["final_cost"] < rep1["initial_cost"]
    st = _three_near(fe, name, end, "after the first solve", strict=False)
    x2, rep2 = fe.setupProblemAndOptimize(x1)
    end = fe.stats()
    assert end["chain_solves"] == st["chain_solves"] + 1 and end["chain_takeovers"] == st["chain_takeovers"], (st, end)
    host = _fe(hip, name)
    host.set_option(_lib.OPT_CHAIN_SOLVE, 0)
    xh, reph = host.setupProblemAndOptimize(x1)
    print("second solve:", x2, rep2, "host-driven, fresh context:", xh, reph)
    assert rel_scalar(rep2["final_cost"], reph["final_cost"]) < RTOL, (rep2, reph)
    assert rel_scalar(-rep2["final_cost"], ref.eval(x2, False)[0]) < RTOL, (x2, rep2)
    assert rel_scalar(-reph["final_cost"], ref.eval(xh, False)[0]) < RTOL, (xh, reph)


def test_warm_solves_on_a_sparse_scene(hip, oracle):
    """The warm end of a device-driven solve (cmx_chain.cpp) hands the next call one dirty plane and a partner it calls clean, with
    the id of the sort the dirty plane's votes were made under.  Solves that end normally, each followed by evaluations: the far
    list of the first test, near points, every other one cost-only.
    The id itself cannot be got wrong on purpose from outside: a queued slot sorts again only when the share reported by the last
    CONSUMED slot passes 3 % (force_rebin comes with a hand-over, which is no warm end), so a skipped slot sorts only if one of
    the last two trial points of a solve that then ends normally crossed that line -- which the line search decides, not the
    caller; on these scenes the share of a converging solve stays under 2 %.  The id is now that of the last executed slot by
    construction (0 if a slot queued behind it sorted again), and this test holds the warm end to the oracle on a sparse scene.
    Every solve must end on the device (no hand-over: only then is the warm end's bookkeeping what the next call sees), and the
    second and third must start warm, the evaluations in between notwithstanding."""
    name = "C"
    ref = sc.fe_oracle(name)
    fe = _fe(hip, name)
    for k in range(3):
        x, rep = fe.setupProblemAndOptimize(OM0)
        st = fe.stats()
        print("solve %d:" % k, x, rep, st)
        assert st["chain_solves"] == k + 1 and st["chain_takeovers"] == 0 and st["chain_warm_starts"] == k, st
        assert rel_scalar(-rep["final_cost"], ref.eval(x, False)[0]) < RTOL, (k, x, rep)
        if k == 0:
            cs, gs = fe.eval_many([sc.far_point(name, OM0)], True)
            c_ref, g_ref = ref.eval(sc.far_point(name, OM0))
            assert rel_scalar(cs[0], c_ref) < RTOL and rel_vec(gs[0], g_ref) < RTOL
        for j in (1, 2, 3, 4):
            _check_eval(fe, name, OM0 + (j + 4 * k) * EPS, "solve %d, near evaluation %d" % (k, j), want_grad=j % 2 == 1)


def test_packets_in_turn(hip, oracle):
    """set_packet(A), evaluations, set_packet(B, the mirror image), evaluations, back to A: what one packet left in the planes --
    far votes included -- must not reach the other, whose active tiles are elsewhere."""
    fe = _fe(hip, "A")
    for rnd, name in enumerate(("A", "B", "A", "C", "B")):
        if rnd:
            _set_packet(fe, name)
        msg = "round %d, packet %s" % (rnd, name)
        _check_eval(fe, name, OM0, msg + ", first evaluation")
        st = fe.stats()
        assert st["rebins"] == rnd + 1
        far = sc.far_point(name, OM0)
        if rnd % 2:
            _check_image(fe, name, far, True, False, msg)
        else:
            c, _ = fe.eval_many([far], False)
            assert rel_scalar(c[0], sc.fe_oracle(name).eval(far, False)[0]) < RTOL, msg
        _check_eval(fe, name, OM0 + EPS, msg + ", near evaluation 1")
        _check_eval(fe, name, OM0 + 2 * EPS, msg + ", near evaluation 2", want_grad=bool(rnd % 2))
        _check_eval(fe, name, OM0 + 2 * EPS, msg + ", the same point again")
        assert fe.stats()["rebins"] == rnd + 1, msg


# ------------------------------------------------------------------------------------------------- seeded walks, front end
def _fe_apply(fe, o):
    """one operation of a walk -> what it returned"""
    k = o["op"]
    if k == "eval":
        c, g = fe.eval(o["x"])
        return {"c": c, "g": g}
    if k == "eval_f":
        return {"c": fe.eval(o["x"], False)[0]}
    if k == "hint_df":      # f = -contrast: scale 0.5 lets the test f < threshold pass (the gradient pass is queued), 2 does not
        fe.hint_next_df(-o["c"] * o["scale"], o["mode"])
        c0 = fe.eval(o["x"], False)[0]
        c, g = fe.eval(o["x"])
        return {"c0": c0, "c": c, "g": g}
    if k in ("eval_many", "eval_each"):
        cs, gs = getattr(fe, k)(o["xs"], o["grad"])
        return {"cs": cs, "gs": gs} if o["grad"] else {"cs": cs}
    if k == "iwe":
        out = fe.computeImageOfWarpedEvents(o["x"], want_deriv=o["deriv"], blur=o["blur"])
        return {"img": out[0], "deriv": out[1]} if o["deriv"] else {"img": out}
    if k == "publish":
        return {"u8": fe.publishEventImage(o["x"])}
    if k == "prepare":
        fe.prepare(o["x"])
    elif k == "set_packet":
        _set_packet(fe, o["packet"])
    elif k == "solve":
        x, rep = fe.setupProblemAndOptimize(o["x"])
        return {"x": x, "initial_cost": rep["initial_cost"], "final_cost": rep["final_cost"]}
    elif k == "option":
        fe.set_option(getattr(_lib, "OPT_" + o["key"]), o["value"])
    else:
        raise KeyError(k)
    return {}


def _fe_check(out, o, msg):
    ref = sc.fe_oracle(o["packet"])
    k = o["op"]
    if "c0" in out:
        assert rel_scalar(out["c0"], o["c"]) < RTOL, (msg, out["c0"], o["c"])
    if k in ("eval", "eval_f", "hint_df"):
        assert rel_scalar(out["c"], o["c"]) < RTOL, (msg, out["c"], o["c"])
        if "g" in out:
            assert rel_vec(out["g"], o["g"]) < RTOL, (msg, out["g"], o["g"])
    elif k in ("eval_many", "eval_each"):
        for i in range(len(o["xs"])):
            assert rel_scalar(out["cs"][i], o["cs"][i]) < RTOL, (msg, i, out["cs"][i], o["cs"][i])
            if o["grad"]:
                assert rel_vec(out["gs"][i], o["gs"][i]) < RTOL, (msg, i, out["gs"][i], o["gs"][i])
    elif k == "iwe":
        r = ref.iwe(o["x"], deriv=o["deriv"], blur=o["blur"])
        assert rel_img(out["img"], r[0] if o["deriv"] else r) < RTOL, msg
        if o["deriv"]:
            for j in range(3):
                assert rel_img(out["deriv"][..., j], r[1][..., j]) < RTOL, (msg, j)
    elif k == "publish":
        dr.assert_within_one(out["u8"], dr.local_pair_levels(ref.iwe(np.zeros(3), blur=False), ref.iwe(o["x"], blur=False)))
    elif k == "solve":
        # the chosen points depend on the last bits of every evaluation; what the report says about its two ends does not
        assert rel_scalar(-out["initial_cost"], ref.eval(o["x"], False)[0]) < RTOL, (msg, out)
        assert rel_scalar(-out["final_cost"], ref.eval(out["x"], False)[0]) < RTOL, (msg, out)
        assert out["final_cost"] <= out["initial_cost"], (msg, out)


@pytest.mark.parametrize("seed", sc.FE_SEEDS)
def test_frontend_walk(hip, oracle, seed):
    ops = sc.fe_walk(seed)
    fe = _fe(hip, ops[0]["packet"])
    for i, o in enumerate(ops):
        msg = "front-end seed %d, step %d\n%s\n%s" % (seed, i, sc.describe(ops, i), fe.stats())
        try:
            out = _fe_apply(fe, o)
        except Exception as e:
            raise AssertionError(msg) from e
        _fe_check(out, o, msg)


def _same_bits(a, b, msg):
    assert a.keys() == b.keys(), msg
    for k in a:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.shape == y.shape and x.tobytes() == y.tobytes(), (msg, k, a[k], b[k])


@pytest.mark.parametrize("seed", sc.FE_DET_SEEDS)
def test_frontend_walk_deterministic_bits(hip, oracle, seed):
    """test_gpu_deterministic.py's promise, extended to arbitrary history: every result of the walk has the bits a fresh
    deterministic context (same packet, same option values) returns for the same call alone -- for an evaluation at the point of
    the evaluation right before it, for the same two calls."""
    ops = sc.fe_walk(seed, True)
    fe = _fe(hip, ops[0]["packet"], True)
    options = {}
    for i, o in enumerate(ops):
        msg = "front-end seed %d (deterministic), step %d\n%s" % (seed, i, sc.describe(ops, i))
        out = _fe_apply(fe, o)
        _fe_check(out, o, msg)
        if o["op"] == "option":
            options[o["key"]] = o["value"]
        if not out:
            continue
        fresh = _fe(hip, o["packet"], True)
        for key, value in options.items():
            fresh.set_option(getattr(_lib, "OPT_" + key), value)
        prev = ops[i - 1] if i else None
        if o["op"] in ("eval", "eval_f") and prev and prev["op"] in ("eval", "eval_f", "hint_df") and np.array_equal(prev["x"], o["x"]):
            _fe_apply(fresh, prev)
        _same_bits(out, _fe_apply(fresh, o), msg)
        fresh.close()


# ------------------------------------------------------------------------------------------------- seeded walks, back end
def _be(hip, which, deterministic=False):
    w = sc.be_window(which)
    be = hip.BackendEvaluator(w.W, w.H, w.lut, w.Wp, w.Hp)
    if deterministic:
        be.set_deterministic()
    return be


def _be_apply(be, o):
    k = o["op"]
    if k == "set_window":
        w = sc.be_window(o["window"])
        be.set_window(w.x, w.y, w.t_ns, w.order, w.knots_init, w.start_ns, w.dt_ns, w.num_fixed, w.t_next_win_beg_ns, w.batch,
                      w.sample_rate, 1.0, _lib.VARIANCE, sc.be_map(o["window"], o["map"]))
    elif k == "eval":
        c, g = be.eval(o["x"])
        return {"c": c, "g": g}
    elif k == "eval_f":
        return {"c": be.eval(o["x"], False)[0]}
    elif k == "hint_df":
        be.hint_next_df(-o["c"] * o["scale"], o["mode"])
        c0 = be.eval(o["x"], False)[0]
        c, g = be.eval(o["x"])
        return {"c0": c0, "c": c, "g": g}
    elif k in ("eval_many", "eval_each"):
        cs, gs = getattr(be, k)(o["xs"], o["grad"])
        return {"cs": cs, "gs": gs} if o["grad"] else {"cs": cs}
    elif k == "plane":
        return {"img": be.get_plane(_lib.PLANE_IL_OLD if o["plane"] == "IL_old" else _lib.PLANE_IL_NEW)}
    elif k == "alpha":
        return {"alpha": be.alpha}
    elif k == "prepare":
        be.prepare(o["x"])
    elif k == "path":
        if o["fast"]:
            be.set_fast_path()
        else:
            be.set_reference_path()
    else:
        raise KeyError(k)
    return {}


def _be_check(out, o, msg):
    k = o["op"]
    if "c0" in out:
        assert rel_scalar(out["c0"], o["c"]) < RTOL, (msg, out["c0"], o["c"])
    if k in ("eval", "eval_f", "hint_df"):
        assert rel_scalar(out["c"], o["c"]) < RTOL, (msg, out["c"], o["c"])
        if "g" in out:
            assert rel_vec(out["g"], o["g"]) < RTOL, (msg, rel_vec(out["g"], o["g"]))
    elif k in ("eval_many", "eval_each"):
        for i in range(len(o["xs"])):
            assert rel_scalar(out["cs"][i], o["cs"][i]) < RTOL, (msg, i, out["cs"][i], o["cs"][i])
            if o["grad"]:
                assert rel_vec(out["gs"][i], o["gs"][i]) < RTOL, (msg, i, rel_vec(out["gs"][i], o["gs"][i]))
    elif k == "plane":
        assert rel_img(out["img"], o["img"]) < RTOL, msg
    elif k == "alpha":
        assert rel_scalar(out["alpha"], o["alpha"]) < RTOL if o["alpha"] else out["alpha"] == 0, (msg, out["alpha"], o["alpha"])


@pytest.mark.parametrize("seed", sc.BE_SEEDS)
def test_backend_walk(hip, oracle, seed):
    ops = sc.be_walk(seed)
    be = _be(hip, ops[0]["window"])
    for i, o in enumerate(ops):
        msg = "back-end seed %d, step %d\n%s" % (seed, i, sc.describe(ops, i))
        try:
            out = _be_apply(be, o)
        except Exception as e:
            raise AssertionError(msg) from e
        _be_check(out, o, msg)


@pytest.mark.parametrize("seed", sc.BE_DET_SEEDS)
def test_backend_walk_deterministic_bits(hip, oracle, seed):
    """The same promise for the back end.  "The same call alone" on a fresh context: the window handed over, the window's first
    evaluation of the walk (the blend factor alpha is fixed there, as in the reference), then the call -- for a plane, the
    evaluation it belongs to; for an evaluation at the point of the evaluation right before it, those two."""
    ops = sc.be_walk(seed, True)
    be = _be(hip, ops[0]["window"], True)
    window = first = last = None
    for i, o in enumerate(ops):
        msg = "back-end seed %d (deterministic), step %d\n%s" % (seed, i, sc.describe(ops, i))
        out = _be_apply(be, o)
        _be_check(out, o, msg)
        k = o["op"]
        if k == "set_window":
            window, first, last = o, None, None
        evaluates = k in ("eval", "eval_f", "hint_df", "eval_many", "eval_each")
        if out:
            fresh = _be(hip, window["window"], True)
            _be_apply(fresh, window)
            if first is not None:
                _be_apply(fresh, first)
            if k in ("plane", "alpha"):
                if last is not first:
                    _be_apply(fresh, last)
            else:
                prev = ops[i - 1]
                if (k in ("eval", "eval_f") and prev is not first and prev["op"] in ("eval", "eval_f", "hint_df") and
                        np.array_equal(prev["x"], o["x"])):
                    _be_apply(fresh, prev)
            _same_bits(out, _be_apply(fresh, o), msg)
            fresh.close()
        if evaluates:
            first = o if first is None else first
            last = o
