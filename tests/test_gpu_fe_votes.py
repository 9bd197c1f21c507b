"""-m gpu: the front-end SPLAT per event, every form of it, against an fp64 warp (tests/fe_probe_cases.py; the inputs and the
comparison are checked on the CPU by tests/test_fe_probe_cases_cpu.py).

A front-end evaluation is splat (events -> forward plane A), image pass (A -> B, Jt, moments), gather (Jt -> gradient).  The last
two are pinned per pixel and per parameter (test_gpu_adjoint_plane.py, test_gpu_gather.py); this file pins the first.  The probe
packets keep every voting event's 2 x 2 cell disjoint from all others with an empty ring around it at every omega of a case, so the
plane IS the list of votes: every cell is held to the fp64 weights of the fp64 warp within

    BOUND = 4 * 2^-24 + 2^-30 = 2.4e-7 absolute

(three fp32 roundings of values <= 1 per weight: the cast of dx, 1 - dx, the product; one 2^-30 fixed-point unit and the cast back on
the LDS and deterministic forms -- from the code's arithmetic, not from a device run), every other pixel to exactly 0, and the plane's
sum to the number of voting events.  The plane is read with forward_plane() (cmx_diag_get_forward_plane): the votes of the context's
LAST splat, so also the fused splat's of an evaluation, which cmx_frontend_get_iwe never shows (it votes again, unfused).

Forms, each with the counter that proves it ran: reference-shaped (fe_splat_kernel, 1 and 4 planes), the adjoint evaluation on
global atomics (SPLAT_MODE 0), FUSED_IMAGE 0 (fe_splat_lds_kernel<.., 0>), the default FUSED_IMAGE 1, FUSED_IMAGE 2
(fe_splat_lds_one_kernel), FUSED_IMAGE 3 (fe_splat_lds_self_kernel), deterministic (the FIXED kernels), and the default options on
a LUT whose z column is not all ones (the STREAM = false kernels).

a. votes at the sort's own parameters: no vote may leave its tile's LDS window (the global path would quietly repair a wrong key);
b. drift: W1, W2 (no vote leaves, no new sort), then W3 -- the number of votes on the global path, or the repeat behind a fresh
   sort, is what the host model of the sort says, exactly;
c. a script of evaluations, cost-only calls, image read-backs and renders on one context, and a packet swap: after every call the
   plane holds that call's votes and exact zeros everywhere else;
d. the derivative planes of fe_splat_kernel<true> per cell.
Every test prints one line per form, case and omega ("FEV|" lines; profiles/fe_votes_parity.txt is a record of them)."""
import numpy as np
import pytest

import fe_probe_cases as fp
from cmax_slam_amd import _lib
from util import RTOL

pytestmark = pytest.mark.gpu

FORMS = {
    "reference-shaped": {},
    "global_atomics": {"splat": 0},
    "three_launches": {"options": (("FUSED_IMAGE", 0),)},
    "default": {},
    "one_launch": {"options": (("FUSED_IMAGE", 2),)},
    "self_serve": {"options": (("FUSED_IMAGE", 3),)},
    "deterministic": {"det": True},
}
SORTED = ["three_launches", "default", "one_launch", "self_serve", "deterministic"]
FUSED = ["default", "one_launch", "self_serve"]
CASE_FORMS = [(name, form) for name in fp.CASES for form in (FORMS if name != "unit_lut" else ["default"])]


def make(hip, form, name, reuse=True):
    p = fp.packet(name)
    fe = (hip.reference_shaped.FrontendEvaluator if form == "reference-shaped" else hip.FrontendEvaluator)(p.W, p.H, p.lut)
    setup = FORMS[form]
    if setup.get("det"):
        fe.set_deterministic()
    for key, value in setup.get("options", ()):
        fe.set_option(getattr(_lib, "OPT_" + key), value)
    if "splat" in setup:
        fe.set_splat_mode(setup["splat"])
    if not reuse:
        fe.set_option(_lib.OPT_REUSE_IMAGE, 0)   # a second evaluation of the same point votes again
    set_packet(fe, name)
    return fe


def set_packet(fe, name):
    p = fp.packet(name)
    fe.set_packet(p.x, p.y, p.t_ns, p.t_ref_ns, p.fx, p.fy, p.cx, p.cy, p.batch, p.sigma, _lib.VARIANCE)


def fallback_count(fe, name):
    st = fe.stats()
    n = len(fp.packet(name).x)
    assert st["events"] == n, st
    return int(round(st["fallback_frac"] * n))


def check_form_ran(form, st, evals):
    """the counters of `evals` gradient evaluations at new points on a fresh context, none of them repeated"""
    msg = (form, evals, st)
    assert st["fused_timeouts"] == 0, msg
    if form in ("reference-shaped", "global_atomics"):
        assert st["rebins"] == 0 and st["fused_evals"] == 0, msg
    elif form in ("three_launches", "deterministic"):
        assert st["rebins"] >= 1 and st["fused_evals"] == 0, msg
    else:
        assert st["rebins"] >= 1 and st["fused_evals"] == evals + st["fused_redos"], msg
        if form == "default":
            assert st["one_launch_evals"] == 0 and st["self_serve_evals"] == 0, msg
        elif form == "one_launch":  # (both expected from the second evaluation of a sort on)
            assert st["one_launch_evals"] >= evals - 1 >= 1 and st["self_serve_evals"] == 0, msg
        else:
            assert st["self_serve_evals"] >= evals - 1 >= 1, msg


def line(kind, form, name, omega, ratio, fe=None, extra=""):
    n = fp.events(name, tuple(omega)).n
    fb = "" if fe is None else ", fallback count %d" % fallback_count(fe, name)
    print("FEV|%s|%s|%s|omega %s|worst cell %.3f bounds, %d voting events%s%s" % (kind, form, name, tuple(omega), ratio, n, fb, extra))


# ------------------------------------------------------------------------------------------------ a. the sort's own parameters
@pytest.mark.parametrize("name,form", CASE_FORMS)
def test_votes_at_the_sorts_own_parameters(hip, name, form):
    for omega in fp.CASES[name].omegas:
        om = np.asarray(omega, np.float64)
        tag = "%s, %s, omega %s" % (form, name, omega)
        fe = make(hip, form, name, reuse=form not in ("one_launch", "self_serve"))
        try:
            if form == "reference-shaped":
                ratio = fp.compare(tag + ", 1 plane", fe.computeImageOfWarpedEvents(om, blur=False), name, omega)
                ratio = max(ratio, fp.compare(tag + ", 1 plane, read back", fe.forward_plane(), name, omega))
                img, _ = fe.computeImageOfWarpedEvents(om, want_deriv=True, blur=False)
                ratio = max(ratio, fp.compare(tag + ", 4 planes", img, name, omega))
                ratio = max(ratio, fp.compare(tag + ", 4 planes, read back", fe.forward_plane(), name, omega))
                c, g = fe.eval(om)
                ratio = max(ratio, fp.compare(tag + ", fdf", fe.forward_plane(), name, omega))
                evals = 1
            else:
                evals = 2 if form in ("one_launch", "self_serve") else 1
                ratio = 0.0
                for k in range(evals):
                    c, g = fe.eval(om)
                    ratio = max(ratio, fp.compare("%s, evaluation %d" % (tag, k), fe.forward_plane(), name, omega))
            assert np.isfinite(c) and np.isfinite(g).all(), (tag, c, g)
            st = fe.stats()
            check_form_ran(form, st, evals)
            if form in SORTED:
                assert st["rebins"] == 1 and st["fused_redos"] == 0 and fallback_count(fe, name) == 0, (tag, st)
            line("own", form, name, omega, ratio, fe if form in SORTED else None)
        finally:
            fe.close()


# ------------------------------------------------------------------------------------------------------- b. drift and fallback
@pytest.mark.parametrize("name,form", [(n, f) for n, f in CASE_FORMS if f in SORTED and n != "far"])
def test_drift_and_fallback_count(hip, name, form):
    fe = make(hip, form, name)
    try:
        for omega in (fp.W1, fp.W2):
            fe.eval(np.asarray(omega))
            ratio = fp.compare("%s, %s, omega %s" % (form, name, omega), fe.forward_plane(), name, omega)
            st = fe.stats()
            assert fallback_count(fe, name) == 0 and st["rebins"] == 1 and st["fused_redos"] == 0, (form, name, omega, st)
            line("drift", form, name, omega, ratio, fe)
        check_form_ran(form, fe.stats(), 2)
        fe.eval(np.asarray(fp.W3))
        ratio = fp.compare("%s, %s, omega %s after %s" % (form, name, fp.W3, fp.W1), fe.forward_plane(), name, fp.W3)
        st = fe.stats()
        want = fp.predicted_fallback(name, fp.W1, fp.W3)
        repeat = form in FUSED and fp.predicted_unsafe(name, fp.W1, fp.W3)
        line("jump", form, name, fp.W3, ratio, fe, "; host model %d, repeat behind a fresh sort: %s; rebins %d, fused_redos %d"
             % (want, repeat, st["rebins"], st["fused_redos"]))
        assert st["fused_timeouts"] == 0, st
        if repeat:   # a vote beyond the tiles' reach: the evaluation was repeated behind a sort at W3, where no vote leaves its window
            assert fallback_count(fe, name) == 0 and st["fused_redos"] == 1 and st["rebins"] == 2, (form, name, st)
        else:
            assert fallback_count(fe, name) == want and st["fused_redos"] == 0 and st["rebins"] == 1, (form, name, want, st)
    finally:
        fe.close()


# --------------------------------------------------------------------------------------------------------- c. nothing stale
SCRIPT = [("eval", fp.W1), ("eval", fp.W2), ("cost", fp.W1), ("eval", fp.W1), ("iwe", fp.W2), ("eval", fp.W2), ("display", fp.W1),
          ("eval", fp.W3), ("eval", fp.W3), ("eval", fp.W0), ("eval", fp.W1)]


def run_script(fe, form, name):
    worst = 0.0
    for step, (call, omega) in enumerate(SCRIPT):
        om = np.asarray(omega, np.float64)
        tag = "%s, %s, step %d: %s at %s" % (form, name, step, call, omega)
        if call == "eval":
            fe.eval(om)
        elif call == "cost":
            fe.eval(om, want_grad=False)
        elif call == "iwe":
            worst = max(worst, fp.compare(tag + ", returned image", fe.computeImageOfWarpedEvents(om, blur=False), name, omega))
        else:
            fe.publishEventImage(om)
        worst = max(worst, fp.compare(tag, fe.forward_plane(), name, omega))
    st = fe.stats()
    assert st["fused_timeouts"] == 0, (form, name, st)
    print("FEV|script|%s|%s|%d calls|worst cell %.3f bounds; rebins %d, fused_evals %d, fused_redos %d, one_launch_evals %d, "
          "self_serve_evals %d" % (form, name, len(SCRIPT), worst, st["rebins"], st["fused_evals"], st["fused_redos"],
                                   st["one_launch_evals"], st["self_serve_evals"]))
    return st


@pytest.mark.parametrize("form", SORTED)
def test_nothing_stale_in_the_plane(hip, form):
    """... and the same script again after set_packet of another packet (other batch size, other events) into the same context,
    then of a packet that votes in one corner only: three quarters of the sort tiles are inactive and whatever the dense packets
    left there, in either ping-pong plane, is cleared by no tile pass"""
    fe = make(hip, form, "qvga")
    try:
        st = run_script(fe, form, "qvga")
        if form in FUSED:
            assert st["fused_evals"] >= 6, st
        if form == "one_launch":     # (at least W2, W2 behind the read-back and W3 under the first sort)
            assert st["one_launch_evals"] >= 3, st
        if form == "self_serve":
            assert st["self_serve_evals"] >= 3, st
        set_packet(fe, "qvga_b257")
        run_script(fe, form, "qvga_b257")
        set_packet(fe, "sparse")
        run_script(fe, form, "sparse")
    finally:
        fe.close()


def test_nothing_stale_on_the_general_lut(hip):
    fe = make(hip, "default", "unit_lut")
    try:
        assert run_script(fe, "default", "unit_lut")["fused_evals"] >= 6
    finally:
        fe.close()


# ------------------------------------------------------------------------------------------------------ d. derivative planes
@pytest.mark.parametrize("name,omega", [("qvga", fp.W1), ("far", fp.FAR_OMEGA)])
def test_derivative_planes_per_cell(hip, name, omega):
    """test_gpu_far_orientations.py's rule: per voting cell, the error relative to the cell's largest magnitude over the three planes"""
    fe = make(hip, "reference-shaped", name)
    try:
        img, d = fe.computeImageOfWarpedEvents(np.asarray(omega, np.float64), want_deriv=True, blur=False)
    finally:
        fe.close()
    ev = fp.events(name, tuple(omega))
    _, mask = fp.reference(name, tuple(omega))
    fp.compare("reference-shaped, %s, 4 planes" % name, img, name, omega)
    assert d.shape == (ev.H, ev.W, 3) and np.isfinite(d).all()
    ys = ev.yy[:, None] + np.array([0, 0, 1, 1])
    xs = ev.xx[:, None] + np.array([0, 1, 0, 1])
    got = np.moveaxis(d[ys, xs, :].astype(np.float64), 2, 0)     # 3 x n x 4
    want = fp.derivative_reference(name, omega)
    scale = np.abs(want).max(axis=(0, 2))
    assert scale.min() > 0
    ratio = np.abs(got - want).max(axis=(0, 2)) / scale
    i = int(np.argmax(ratio))
    print("FEV|deriv|reference-shaped|%s|omega %s|largest per-cell ratio %.2e (cell scale %.3g .. %.3g), %d voting events"
          % (name, tuple(omega), ratio[i], scale.min(), scale.max(), ev.n))
    assert ratio[i] < RTOL, (name, int(ev.src[i]), ratio[i], got[:, i], want[:, i])
    assert not d[~mask].any()


# ------------------------------------------------------------------------------------------------------------- the read-back
def test_forward_plane_read_back_states_and_errors(hip):
    L = _lib.lib()
    p = fp.packet("one_tile_row")
    buf = np.zeros((p.H, p.W), np.float32)
    ptr = buf.ctypes.data_as(_lib.c_fp)

    def status(fn):
        try:
            fn()
        except hip.CmaxHipError as e:
            return e.status
        return _lib.OK

    fe = hip.FrontendEvaluator(p.W, p.H, p.lut)
    try:
        assert status(fe.forward_plane) == _lib.ERR_STATE                       # no packet
        set_packet(fe, "one_tile_row")
        assert status(fe.forward_plane) == _lib.ERR_STATE                       # no accumulate of this packet yet
        c0, g0 = fe.eval(np.asarray(fp.W1))
        assert L.cmx_diag_get_forward_plane(fe._ctx, None) == _lib.ERR_INVALID_ARG
        st = fe.stats()
        a, b = fe.forward_plane(), fe.forward_plane()                           # reading changes nothing and launches nothing
        assert np.array_equal(a, b) and fe.stats() == st
        c1, g1 = fe.eval(np.asarray(fp.W2))
        fe.forward_plane()
        c2, g2 = fe.eval(np.asarray(fp.W1))
        assert c2 == pytest.approx(c0, rel=1e-12) and fe.stats()["fused_redos"] == 0
        set_packet(fe, "one_tile_row")
        assert status(fe.forward_plane) == _lib.ERR_STATE                       # a new packet: the plane belongs to no evaluation of it
    finally:
        fe.close()
    assert L.cmx_diag_get_forward_plane(None, ptr) == _lib.ERR_INVALID_ARG
    be = hip.BackendEvaluator(p.W, p.H, p.lut, 256, 128)
    try:
        assert L.cmx_diag_get_forward_plane(be._ctx, ptr) == _lib.ERR_STATE     # front-end contexts only
    finally:
        be.close()
    grp = hip.BackendEvaluator(p.W, p.H, p.lut, 256, 128, devices=[0, 0])
    try:
        assert L.cmx_diag_get_forward_plane(grp._ctx, ptr) == _lib.ERR_INVALID_ARG
    finally:
        grp.close()
