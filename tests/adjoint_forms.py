"""Test helper: every form of an adjoint evaluation, once, on one small front-end scene and one small back-end window.

An adjoint evaluation is queued in five forms (cmx_pipeline.cpp: adjoint_eval, adjoint_partial_sums, adjoint_finalize_sums,
adjoint_cost_only, adjoint_gated_grad); options, the contrast measure, the size of the panorama and what the context holds from
the call before decide which steps each of them launches.  FORMS lists the call sequences that reach every one of those choices.
walk() runs them, each on a fresh context, and reports per form what the calls returned, what the oracle returns for the same
arguments (stateless: tests/seq_cases.py), the launches per class that timing_get counts and what stats() counted.

Used by tests/test_gpu_adjoint_forms.py (which asserts all of it) and by tools/adjoint_forms_walk.py (which prints it, for a
comparison of two builds of the library).  Scenes, points and expected values come from the oracle and cmax_slam_amd.synth alone.
"""
import functools

import numpy as np

import seq_cases as sc
from cmax_slam_amd import _lib, synth
from oracle import pyoracle as po

CLASSES = ("image", "gather", "final", "batch")
STATS = ("spec_images", "spec_hits", "gated_launches", "gated_hits", "reuse_hits", "host_finalize_evals")
CHAIN_STATS = ("chain_solves", "chain_takeovers", "chain_warm_starts")

FE_X = (sc.OMEGA0, sc.OMEGA0 + np.array([0.10, -0.05, 0.08]))


@functools.lru_cache(maxsize=None)
def be_window(scene):
    """'small': seq_cases.be_window(0).  'big': the same camera and spline on a 2048 x 1056 panorama, 2112 tiles of 64 x 16 --
    just above kTileListMin = 2048, where the image pass takes a compacted tile list (not in deterministic mode)."""
    if scene == "big":
        return synth.backend_window(25_000, sc.W, sc.H, sc.FX, sc.FY, sc.CX, sc.CY, 2048, 1056, 2, 5, 1, 0.2, seed=75)
    return sc.be_window(0)


def be_points(scene):
    P = be_window(scene).P
    return 0.01 * np.cos(np.arange(P)), 0.01 * np.sin(1.0 + np.arange(P))


# name -> (kinds it applies to, script, set-up).  Scripts:
#   f_df      eval(x0, cost only), eval(x1)                         a df at a new point
#   f_df_same eval(x0, cost only), eval(x0)                         ... at the same point: the resident image is reused
#   hint      hint_next_df, eval(x0, cost only), eval(x0)           scale 0.5: f = -contrast passes f < threshold (gate open), 2: shut
#   many      eval_many([x0, x1])
#   split     accumulate(x0), finish_begin, finish_end              the caller's all-reduce of the 2P-double buffer would sit in between
#   three     eval(x0, cost only), eval(x0), eval(x1)               what the option forms run
#   solve     setupProblemAndOptimize(x0)                           untimed: a timed context does not chain
FORMS = {
    "f_df_new": ("fb", "f_df", {}),
    "f_df_same": ("fb", "f_df_same", {}),
    "hint_open": ("fb", "hint", {"scale": 0.5}),
    "hint_shut": ("fb", "hint", {"scale": 2.0}),
    "eval_many": ("fb", "many", {}),
    "split_2p": ("fb", "split", {}),
    "split_rows": ("fb", "three", {"comm": True}),   # a communicator of world size 1: the accumulator-row split
    "deterministic": ("fb", "three", {"det": True}),
    "tail_0": ("fb", "three", {"options": (("TAIL_FINALIZE", 0),)}),
    "tail_1": ("fb", "three", {"options": (("TAIL_FINALIZE", 1),)}),
    "tail_2": ("fb", "three", {"options": (("TAIL_FINALIZE", 2),)}),
    "tail_4": ("fb", "three", {"options": (("TAIL_FINALIZE", 4),)}),
    "empty": ("fb", "three", {"scene": "empty"}),
    "fold_0": ("b", "three", {"options": (("FOLD_BATCH", 0),)}),
    "big": ("b", "three", {"scene": "big"}),
    "big_deterministic": ("b", "three", {"scene": "big", "det": True}),
    "gradmag": ("f", "three", {"measure": _lib.GRADIENT_MAGNITUDE}),
    "solve_default": ("f", "solve", {}),
    "solve_4": ("f", "solve", {"options": (("CHAIN_SOLVE", 4),)}),
}
DETERMINISTIC = tuple(n for n, f in FORMS.items() if f[2].get("det"))


def forms(kind):
    return [n for n, f in FORMS.items() if kind in f[0]]


# ------------------------------------------------------------------------------------------------- the oracle's side
@functools.lru_cache(maxsize=None)
def _fe_oracle(scene, measure):
    p = sc.packet("A")
    n = 0 if scene == "empty" else len(p.x)
    ref = po.Frontend(p.W, p.H, p.lut, p.fx, p.fy, p.cx, p.cy, p.batch, p.sigma, measure)
    ref.set_packet(p.x[:n], p.y[:n], p.t_ns[:n], p.t_ref_ns)
    return ref


@functools.lru_cache(maxsize=None)
def _be_oracle(scene):
    w = be_window("small" if scene == "empty" else scene)
    n = 0 if scene == "empty" else len(w.x)
    ref = po.Backend(w.W, w.H, w.lut, w.Wp, w.Hp, w.order, w.batch, w.sample_rate, 1.0, po.VARIANCE)
    ref.set_window(w.x[:n], w.y[:n], w.t_ns[:n], w.knots_init, w.start_ns, w.dt_ns, w.num_fixed, w.t_next_win_beg_ns, None)
    return ref


@functools.lru_cache(maxsize=None)
def expected(kind, name, i):
    """(contrast, gradient) of the oracle at point i of a form's scene.  No global map: the back end's blend factor is 0 whatever
    the order of the evaluations.  An empty scene has contrast 0 and gradient 0 by definition (no vote, no image)."""
    setup = FORMS[name][2]
    scene = setup.get("scene", "small")
    if kind == "f":
        c, g = _fe_oracle(scene, setup.get("measure", po.VARIANCE)).eval(FE_X[i])
    elif scene == "empty":
        return 0.0, np.zeros(be_window("small").P)
    else:
        c, g = _be_oracle(scene).eval(be_points(scene)[i], True)
    return float(c), np.asarray(g, np.float64)


# ------------------------------------------------------------------------------------------------- the library's side
def _identity_allreduce(buf, count, dt, op, stream):
    return 0   # world size 1: the sum over the ranks is what is there


def make_context(hip, kind, name):
    setup = FORMS[name][2]
    scene = setup.get("scene", "small")
    if kind == "f":
        p = sc.packet("A")
        n = 0 if scene == "empty" else len(p.x)
        ev = hip.FrontendEvaluator(p.W, p.H, p.lut)
    else:
        w = be_window("small" if scene == "empty" else scene)
        n = 0 if scene == "empty" else len(w.x)
        ev = hip.BackendEvaluator(w.W, w.H, w.lut, w.Wp, w.Hp)
    if setup.get("det"):
        ev.set_deterministic()
    for key, value in setup.get("options", ()):
        ev.set_option(getattr(_lib, "OPT_" + key), value)
    if kind == "f":
        ev.set_packet(p.x[:n], p.y[:n], p.t_ns[:n], p.t_ref_ns, p.fx, p.fy, p.cx, p.cy, p.batch, p.sigma,
                      setup.get("measure", _lib.VARIANCE))
    else:
        ev.set_window(w.x[:n], w.y[:n], w.t_ns[:n], w.order, w.knots_init, w.start_ns, w.dt_ns, w.num_fixed, w.t_next_win_beg_ns,
                      w.batch, w.sample_rate, 1.0, _lib.VARIANCE, None)
    if setup.get("comm"):
        ev.comm_attach_custom(_identity_allreduce, 0, 1)
    return ev


def run_script(ev, kind, name):
    """the calls of a form -> [(point index, contrast, gradient or None), ...] in call order"""
    _, script, setup = FORMS[name]
    scene = setup.get("scene", "small")
    x = FE_X if kind == "f" else be_points("small" if scene == "empty" else scene)
    out = []

    def call(i, want_grad):
        c, g = ev.eval(x[i], want_grad)
        out.append((i, float(c), np.array(g, np.float64) if want_grad else None))

    if script == "f_df":
        call(0, False), call(1, True)
    elif script == "f_df_same":
        call(0, False), call(0, True)
    elif script == "hint":
        ev.hint_next_df(-expected(kind, name, 0)[0] * setup["scale"], 1)
        call(0, False), call(0, True)
    elif script == "many":
        cs, gs = ev.eval_many(np.array([x[0], x[1]]), True)
        out.extend((i, float(cs[i]), np.array(gs[i], np.float64)) for i in (0, 1))
    elif script == "split":
        ev.accumulate(x[0], True)
        ev.finish_begin(True)
        c, g = ev.finish_end(True)
        out.append((0, float(c), np.array(g, np.float64)))
    elif script == "three":
        call(0, False), call(0, True), call(1, True)
    else:
        raise KeyError(script)
    return out


def run_form(hip, kind, name, timed=True):
    """One form on a fresh context.  Returns {'results': [(i, c, g)], 'launches': {class: n}, 'stats': {counter: delta}}; a solve
    form returns {'x', 'final_cost', 'stats'} with the chain counters and runs untimed."""
    ev = make_context(hip, kind, name)
    try:
        if FORMS[name][1] == "solve":
            before = ev.stats()
            xs, rep = ev.setupProblemAndOptimize(FE_X[0])
            after = ev.stats()
            return {"x": np.array(xs, np.float64), "final_cost": float(rep["final_cost"]),
                    "stats": {k: after[k] - before[k] for k in CHAIN_STATS + ("chain_slots",)}}
        if timed:
            ev.timing_enable(CLASSES)
            ev.timing_get()
        before = ev.stats()
        results = run_script(ev, kind, name)
        after = ev.stats()
        launches = {k: v[1] for k, v in ev.timing_get().items() if k in CLASSES} if timed else {}
        return {"results": results, "launches": launches, "stats": {k: after[k] - before[k] for k in STATS}}
    finally:
        ev.close()


def walk(hip, timed=True, only=None):
    """(kind, form name, run_form's record) for every form of both kinds, front end first"""
    for kind in "fb":
        for name in forms(kind):
            if only is None or name in only:
                yield kind, name, run_form(hip, kind, name, timed)
