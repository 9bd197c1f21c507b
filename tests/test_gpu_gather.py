"""-m gpu: the gradient GATHER per parameter against an fp64 gather on the host that reads the device's own Jt (tests/gather_ref.py).

The image pass leaves the plane Jt (pinned per pixel by tests/test_gpu_adjoint_plane.py); the gather reads it at every event's vote
cell, multiplies by the event's pixel Jacobian, sums per batch, maps every batch through its spline Jacobian onto the knot parameters
and the finalize forms (2/N)(S1 - mu S2).  The other tests see that half through rel_vec(g, g_oracle) < RTOL: the max-norm error of
the whole vector against an fp32 oracle.  Here, per case: a fresh context, ONE evaluation with gradient, then Jt and the forward plane
are read back, the host repeats the gather in fp64 over that Jt and

    |g_dev,k - g_ref,k| <= bound_k = 8 max(e32_k, 2^-24 M_k)        for every parameter k,

e32_k the distance of the same sums with the per-event factors formed in fp32 as the kernels form them, M_k the sum of the magnitudes
of the terms added into k -- both from the reference side alone.  The inputs (tests/gather_cases.py) put every batch in a knot
segment of its own, so an event filed under the neighbouring batch, a dropped or doubled event at a slice end, a wrong border term
or a wrong knot each exceed the bound thousands of times over in some parameter (tests/test_gather_ref_cpu.py shows that on the CPU).
The gather forms are selected as tests/adjoint_forms.py selects them: defaults, deterministic mode, FOLD_BATCH 0, TAIL_FINALIZE
0 / 1 / 2 / 4, the global-atomics splat.  Every test prints one line per evaluation: device error over bound (worst parameter),
e32 over M, events, parameters.  Device figures: profiles/gather_parity.txt.

The reference-shaped evaluator (derivative planes) has no Jt and no gather, so it is not among the forms.  Found here: with more than
42 free knots the tail finalize of the back-end gathers summed only the first 256 of its 2 gP accumulator columns and took the S2
sums of the last knots from uninitialised LDS (cases o2_b28 and, independent of what LDS holds, seam_61_knots)."""
import numpy as np
import pytest

import gather_cases as gc
import gather_ref as gr
from cmax_slam_amd import _lib

pytestmark = pytest.mark.gpu

FORMS = {
    "defaults": {},
    "deterministic": {"det": True},
    "fold_0": {"options": (("FOLD_BATCH", 0),)},
    "tail_0": {"options": (("TAIL_FINALIZE", 0),)},
    "tail_1": {"options": (("TAIL_FINALIZE", 1),)},
    "tail_2": {"options": (("TAIL_FINALIZE", 2),)},
    "tail_4": {"options": (("TAIL_FINALIZE", 4),)},
    "global_atomics": {"splat": 0},
}
FE_FORMS = [f for f in FORMS if f != "fold_0"]  # (FOLD_BATCH is a back-end option)


def configure(ev, form):
    setup = FORMS[form]
    if setup.get("det"):
        ev.set_deterministic()
    for key, value in setup.get("options", ()):
        ev.set_option(getattr(_lib, "OPT_" + key), value)
    if "splat" in setup:
        ev.set_splat_mode(setup["splat"])


def check(tag, ev, g_dev, Jt, A, sigma, measure, first_param=0):
    """the per-parameter comparison and the test's printed line"""
    g_dev = np.asarray(g_dev, np.float64)
    assert g_dev.shape == (ev.P,), (tag, g_dev.shape, ev.P)
    assert np.isfinite(g_dev).all(), tag
    cells = (Jt[ev.yy, ev.xx], Jt[ev.yy, ev.xx + 1], Jt[ev.yy + 1, ev.xx], Jt[ev.yy + 1, ev.xx + 1])
    assert all(np.isfinite(c).all() for c in cells), "%s: Jt is not finite at a vote cell" % tag
    ref = gr.gather(ev, Jt, A, sigma, measure)
    k, ratio = gr.worst(g_dev, ref)
    nz = ref.M > 0
    print("gather %s: device error over bound %.3f (parameter %d), e32 over M %.2e, events %d, parameters %d; |g|max %.4g, border events %d"
          % (tag, ratio, k + first_param, float((ref.e32[nz] / ref.M[nz]).max()) if nz.any() else 0.0, ev.n, ev.P,
             float(np.abs(ref.g).max()), ref.n_edge))
    assert ev.n == 0 or np.abs(ref.g).max() > 0, tag
    assert ratio <= 1.0, "%s: %s" % (tag, gr.describe(ev, ref, g_dev, k, first_param))
    return ref


# ---------------------------------------------------------------------------------------------------------------- front end
def fe_one(hip, tag, p, omega, sigma, measure=0, form="defaults"):
    ev = gc.fe_events(p, omega)
    fe = hip.FrontendEvaluator(p.W, p.H, p.lut)
    try:
        configure(fe, form)
        fe.set_packet(p.x, p.y, p.t_ns, p.t_ref_ns, p.fx, p.fy, p.cx, p.cy, p.batch, sigma, measure)
        c, g = fe.eval(np.asarray(omega, np.float64))
        Jt = fe.adjoint_plane()
        A = fe.computeImageOfWarpedEvents(np.asarray(omega, np.float64), blur=False)
    finally:
        fe.close()
    assert abs(float(A.sum(dtype=np.float64)) - ev.n) <= 1e-4 * max(ev.n, 1), "%s: the host's voting events are not the device's" % tag
    return check("front end %s, omega %s, sigma %g, measure %d [%s]" % (tag, tuple(omega), sigma, measure, form), ev, g, Jt, A, sigma,
                 measure)


@pytest.mark.parametrize("kind", ["exact", "band", "corners", "last"])
def test_front_end_packets(hip, kind):
    """integer cells; every event in the border band; in the four corners; on the last accepted cells -- at omega = 0 and off it"""
    for omega in gc.FE_OMEGAS:
        ref = fe_one(hip, kind, gc.fe_packet(kind, 1.0), omega, 1.0)
        if kind in ("band", "corners"):
            assert ref.n_edge > 100 and np.abs(ref.S2).max() > 0


@pytest.mark.parametrize("n", gc.FE_COUNTS)
def test_front_end_event_counts(hip, n):
    """slice ends: one event, one short of / exactly / one past a workgroup's stride and the four-event phases, 2^16 + 1, and the
    largest packet below the slice rule's change"""
    for omega in gc.FE_OMEGAS:
        fe_one(hip, "%d events" % n, gc.fe_packet("count", 1.0, n), omega, 1.0)


@pytest.mark.parametrize("kind,sigma", [("band", 0.0), ("band", 2.0), ("corners", 2.0)])
def test_front_end_band_width(hip, kind, sigma):
    """sigma 0 (no band, Jt is the plane itself) and 2 (r = 7): the border term's condition moves with r"""
    for omega in gc.FE_OMEGAS:
        fe_one(hip, kind, gc.fe_packet(kind, sigma), omega, sigma)


def test_front_end_other_measures(hip):
    """MEAN_SQUARE has no mu term; GRADIENT_MAGNITUDE reads the Sobel Jt and has none either"""
    for measure in (1, 2):
        fe_one(hip, "corners", gc.fe_packet("corners", 1.0), gc.FE_OMEGAS[1], 1.0, measure)
        fe_one(hip, "1025 events", gc.fe_packet("count", 1.0, 1025), gc.FE_OMEGAS[1], 1.0, measure)


@pytest.mark.parametrize("form", [f for f in FE_FORMS if f != "defaults"])
def test_front_end_forms(hip, form):
    for tag, p in (("corners", gc.fe_packet("corners", 1.0)), ("257 events", gc.fe_packet("count", 1.0, 257)),
                   ("65537 events", gc.fe_packet("count", 1.0, 65_537))):
        fe_one(hip, tag, p, gc.FE_OMEGAS[1], 1.0, form=form)


# ------------------------------------------------------------------------------------------------------- back-end window
def be_one(hip, name, form="defaults"):
    c, x, y, t, lut, knots, start_ns, dt_ns, _, IG, side = gc.be_case("window", name)
    ev = gc.be_events("window", name)
    W, H = gc.SENSOR[:2]
    be = hip.BackendEvaluator(W, H, lut, c["Wp"], c["Hp"])
    try:
        configure(be, form)
        be.set_window(x, y, t, c["order"], knots, start_ns, dt_ns, c["nf"], side, c["per_batch"], c["rate"], c["sigma"], c["measure"], IG)
        con, g = be.eval(gc.be_point("window", name))
        Jt = be.adjoint_plane()
        old, new, alpha = be.get_plane(_lib.PLANE_IL_OLD), be.get_plane(_lib.PLANE_IL_NEW), be.alpha
    finally:
        be.close()
    votes = old + new
    assert abs(float(votes.sum(dtype=np.float64)) - ev.n) <= 1e-4 * ev.n, "window %s: the host's voting events are not the device's" % name
    A = votes
    if IG is not None:
        assert alpha > 0, alpha
        A = IG * np.float32(alpha) + votes
    if c["side"] is not None:
        assert old.any() and new.any()
    return check("window %s: order %d, per_batch %d, rate %d, num_fixed %d [%s]" % (name, c["order"], c["per_batch"], c["rate"], c["nf"],
                                                                                    form), ev, g, Jt, A, c["sigma"], c["measure"],
                 3 * c["nf"])


@pytest.mark.parametrize("name", gc.PER_BATCH_CASES)
def test_window_batch_sizes(hip, name):
    be_one(hip, name)


@pytest.mark.parametrize("name", [n for n in gc.WINDOW if n not in gc.PER_BATCH_CASES])
def test_window_edges(hip, name):
    """a last batch of one event, a sampling rate above 1, num_fixed 1 and mid-spline, a map handed in, both sides of
    t_next_win_beg_ns, MEAN_SQUARE at sigma 2"""
    be_one(hip, name)


@pytest.mark.parametrize("form", [f for f in FORMS if f != "defaults"])
def test_window_forms(hip, form):
    for name in gc.FORM_CASES:
        be_one(hip, name, form)


# ------------------------------------------------------------------------------------------------------ whole trajectory
def recon_one(hip, name, route, det=False, frozen=0):
    """route 'add': begin, add, contrast, grad_add, grad_get; 'bound': bind + eval_bound (frozen > 0: behind freeze_head)"""
    c, x, y, t, lut, knots, start_ns, dt_ns, _, _, _ = gc.be_case("recon", name)
    ev = gc.be_events("recon", name, frozen)
    W, H = gc.SENSOR[:2]
    be = hip.BackendEvaluator(W, H, lut, c["Wp"], c["Hp"])
    store = None
    try:
        if det:
            be.set_deterministic()
        be.reconstruct_begin(c["order"], knots, start_ns, dt_ns, c["per_batch"], c["rate"])
        if route == "add":
            be.reconstruct_add(x, y, t)
            be.reconstruct_contrast(c["sigma"], c["measure"], want_grad=True)
            be.reconstruct_grad_add(x, y, t)
            g = be.reconstruct_grad_get()
        else:
            store = hip.EventStore(W, H, len(x))
            store.push(x, y, t)
            be.reconstruct_bind(store, 0, len(x))
            if frozen:
                be.reconstruct_freeze_head(frozen)
                assert be.reconstruct_frozen_info()["frozen_batches"] > 0
            _, g = be.reconstruct_eval_bound(None, c["sigma"], c["measure"])
        Jt = be.reconstruct_adjoint_plane()
        A = be.reconstruct_get()
    finally:
        be.close()
        if store is not None:
            store.close()
    full = gc.be_events("recon", name)
    assert abs(float(A.sum(dtype=np.float64)) - full.n) <= 1e-4 * full.n, "%s: the host's voting events are not the device's" % name
    assert g.shape == (3 * len(knots),)
    tag = "whole trajectory %s: order %d, per_batch %d, K %d [%s%s%s]" % (name, c["order"], c["per_batch"], len(knots), route,
                                                                        ", deterministic" if det else "",
                                                                        ", frozen head %d" % frozen if frozen else "")
    return check(tag, ev, g[3 * frozen:], Jt, A, c["sigma"], c["measure"], 3 * frozen)


@pytest.mark.parametrize("det", [False, True])
@pytest.mark.parametrize("name", list(gc.RECON))
def test_whole_trajectory(hip, name, det):
    recon_one(hip, name, "add", det)


@pytest.mark.parametrize("name", list(gc.RECON))
def test_whole_trajectory_bound(hip, name):
    recon_one(hip, name, "bound")


@pytest.mark.parametrize("name,frozen", [("long4", 150), ("long2", 150), ("run_ends", 31), ("gap", 8)])
def test_whole_trajectory_frozen_head(hip, name, frozen):
    """the line cuts the knots of the batches in segments frozen - order + 1 .. frozen - 1: their columns below it are dropped"""
    order = gc.RECON[name]["order"]
    ev = gc.be_events("recon", name, frozen)
    cut = (ev.col0 < 0) & (ev.col0 + 3 * order > 0)
    assert cut.sum() == order - 1
    recon_one(hip, name, "bound", frozen=frozen)
