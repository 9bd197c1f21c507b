"""CPU: the fp64 gather reference (tests/gather_ref.py) and the inputs of the per-parameter gather tests (tests/gather_cases.py).

1. Fed with dense_image_ops.jt_ref of the all-fp64 image, the reference reproduces the gradient of the all-fp64 oracle
   (FrontendExact / BackendExact) at cases where the suite already trusts it.  The accuracy asked for is what the reference's inputs
   allow, per parameter: Jt is handed over as a plane whose pixels are trusted to dense_image_ops.bound's b, and A_e, B_e are
   combinations of two pixel differences with weights that sum to one, so |dA_e|, |dB_e| <= 2 b and the gradient moves by at most
   jt_k = (2/N) 2 b sum_e (|J_e| |Jb|)_k; the offsets dx, dy and the Jacobian blocks enter the reference rounded to fp32, which
   bound_k covers.  tol_k = jt_k + bound_k.  A wrong Jacobian, scatter, border term or mean is an error of the order of M_k.
2. Every mutation of the reference's own event list -- one event filed under the next batch, one event dropped, one border term
   skipped, one batch's columns shifted by a knot -- exceeds FOUR times bound_k at some parameter, in every case meant to catch it.
3. The same mutations at cases A and B of recon_cases.py against the present comparison, rel_vec(g, g') < RTOL: how many it misses.
Figures: profiles/gather_parity.txt."""
import numpy as np
import pytest

import dense_image_ops as dio
import gather_cases as gc
import gather_ref as gr
import recon_cases as rc
import recon_grad_cases as rg
from cmax_slam_amd import synth
from util import RTOL, rel_vec

CATCH = 4.0  # a mutation must reach this many bounds; if it does not, the inputs are wrong -- not this factor


def host_planes(ev, sigma, measure):
    """(Jt fp32, A) of an EventList without a device: the host's fp32 votes and dense_image_ops.jt_ref of them"""
    A = gr.forward_plane(ev)
    return dio.jt_ref(A, sigma, measure).astype(np.float32), A


def jt_tolerance(ev, b):
    """(2/N) 2 b sum_e (|J_e,0| + |J_e,1|) |Jb| per parameter: what a per-pixel error b of Jt can do to the gradient"""
    return 2.0 / (ev.W * ev.H) * 2.0 * b * gr._magnitudes(ev, np.abs(ev.J64[:, 0, :]) + np.abs(ev.J64[:, 1, :]))


def check_against_exact(tag, ev, g_exact, sigma, measure):
    A = gr.forward_plane(ev, exact=True)
    J = dio.jt_ref(A, sigma, measure)
    b, e32, scale = dio.bound(A, sigma, measure, J)
    ref = gr.gather(ev, J.astype(np.float32), A, sigma, measure)
    tol = jt_tolerance(ev, b) + ref.bound
    err = np.abs(ref.g - g_exact)
    k = int(np.argmax(err / np.where(tol > 0, tol, 1.0)))
    print("gather_ref vs exact %s: worst parameter %d, |difference| %.3e = %.3f tol (tol %.3e = %.2e M), rel_vec %.2e, %d events, "
          "%d parameters" % (tag, k, err[k], err[k] / tol[k], tol[k], tol[k] / ref.M[k], rel_vec(ref.g, g_exact), ev.n, ev.P))
    assert np.abs(g_exact).max() > 0
    assert (err <= tol).all(), (tag, k, gr.describe(ev, ref, g_exact, k))


@pytest.mark.parametrize("name,sigma", [("pano130x96", 1.0), ("window", 1.0), ("B", 1.0), ("window", 2.0), ("pano130x96", 0.0)])
def test_reference_reproduces_the_fp64_back_end(oracle, name, sigma):
    c, (w, x, y, t) = rc.CASES[name], rc.window(name)
    q = rg.point(name)
    ev = gr.be_events(x, y, t, w.lut, rc.SENSOR[0], c["Wp"], c["Hp"], c["order"], q, w.start_ns, w.dt_ns, 0, c["batch"], c["rate"])
    assert ev.n > 0.9 * rc.sampled(c["N"], c["batch"], c["rate"])
    for measure in (0, 1):
        _, g = rg.oracle_eval(oracle, name, x, y, t, q, sigma, measure, exact=True)
        check_against_exact("%s sigma %g measure %d" % (name, sigma, measure), ev, g, sigma, measure)


def test_reference_respects_num_fixed(oracle):
    name, nf = "window", 4
    c, (w, x, y, t) = rc.CASES[name], rc.window(name)
    q = rg.point(name)
    ev = gr.be_events(x, y, t, w.lut, rc.SENSOR[0], c["Wp"], c["Hp"], c["order"], q, w.start_ns, w.dt_ns, nf, c["batch"], c["rate"])
    _, g = rg.oracle_eval(oracle, name, x, y, t, q, 1.0, 0, exact=True, num_fixed=nf)
    assert ev.P == len(g) == 3 * (c["K"] - nf) and (ev.col0 < 0).any()
    check_against_exact("window num_fixed %d" % nf, ev, g, 1.0, 0)


@pytest.mark.parametrize("sigma,measure", [(1.0, 0), (1.0, 1), (2.0, 0), (0.0, 0), (1.0, 2)])
def test_reference_reproduces_the_fp64_front_end(oracle, sigma, measure):
    p = synth.frontend_packet(8000, 120, 90, 100.0, 100.0, 59.5, 44.5, seed=3)
    omega = 0.7 * p.omega_true
    ex = oracle.FrontendExact(p.W, p.H, p.lut, p.fx, p.fy, p.cx, p.cy, p.batch, sigma, measure)
    ex.set_packet(p.x, p.y, p.t_ns, p.t_ref_ns)
    _, g = ex.eval(omega)
    ev = gr.fe_events(p, omega)
    assert ev.n > 6000
    check_against_exact("front end sigma %g measure %d" % (sigma, measure), ev, g, sigma, measure)


# ---------------------------------------------------------------------------------------------------------------- mutations
def free_batches(ev):
    """batches with every column on a parameter"""
    C = ev.Jb.shape[2]
    return np.nonzero((ev.col0 >= 0) & (ev.col0 + C <= ev.P))[0]


def heaviest(ev, Jt, among):
    w = gr.weight(ev, Jt)
    return int(among[np.argmax(w[among])])


def mutations_of(ev, Jt, r, batches=None):
    """[(name, mutated list)]: the mutations that apply to the list"""
    out = []
    nb = len(ev.col0)
    if nb > 1:
        fb = free_batches(ev)
        fb = fb[fb + 1 < nb]
        for b in ([int(fb[len(fb) // 2])] if batches is None else batches):
            in_b = np.nonzero(ev.batch == b)[0]
            out.append(("next batch [%d]" % b, gr.mutate_next_batch(ev, heaviest(ev, Jt, in_b))))
            out.append(("columns shifted [%d]" % b, gr.mutate_shift_columns(ev, b)))
            if batches is not None:
                out.append(("dropped [%d]" % b, gr.mutate_drop(ev, heaviest(ev, Jt, in_b))))
    if batches is None:
        tail = np.arange(max(0, ev.n - 64), ev.n)  # (a slice end: the ragged last lane group)
        if nb > 1:
            tail = tail[np.isin(ev.batch[tail], free_batches(ev))]
        out.append(("dropped", gr.mutate_drop(ev, heaviest(ev, Jt, tail))))
    return out


def mutation_ratios(tag, ev, sigma, measure, extra=()):
    Jt, A = host_planes(ev, sigma, measure)
    ref = gr.gather(ev, Jt, A, sigma, measure)
    rows = []
    for name, mut in mutations_of(ev, Jt, dio.radius(sigma)) + list(extra):
        g = gr.gather_value(mut, Jt, ref.mu, sigma, measure)
        d = np.abs(g - ref.g)
        k = int(np.argmax(d / np.where(ref.bound > 0, ref.bound, 1e-300)))
        rows.append((name, d[k] / max(ref.bound[k], 1e-300), k, rel_vec(g, ref.g)))
    print("gather mutations %s (%d events, %d parameters): %s" %
          (tag, ev.n, ev.P, "; ".join("%s %.3g bounds at parameter %d (rel_vec %.1e)" % row for row in rows)))
    for name, ratio, k, _ in rows:
        assert ratio >= CATCH, "%s: '%s' reaches %.3g bounds only (parameter %d): the inputs do not separate it" % (tag, name, ratio, k)
    return rows


@pytest.mark.parametrize("name", list(gc.WINDOW))
def test_window_cases_catch_every_mutation(oracle, name):
    c = gc.WINDOW[name]
    ev = gc.be_events("window", name)  # (asserts the layout: batch b in its segment, no coordinate near an integer)
    assert np.array_equal(ev.col0, 3 * (ev.info["segment"] - c["nf"]))
    rows = mutation_ratios("window " + name, ev, c["sigma"], c["measure"])
    assert len(rows) == 3


@pytest.mark.parametrize("name", list(gc.RECON))
def test_whole_trajectory_cases_catch_every_mutation(oracle, name):
    c = gc.RECON[name]
    ev = gc.be_events("recon", name)
    if len(ev.col0) > 1:
        assert len(mutation_ratios("whole trajectory " + name, ev, c["sigma"], c["measure"])) == 3
    else:
        mutation_ratios("whole trajectory " + name, ev, c["sigma"], c["measure"])
    # the frozen head of the bound evaluation: the same list with the line through the middle
    K = len(gc.be_case("recon", name)[5])
    evf = gc.be_events("recon", name, K // 2)
    assert evf.P == 3 * (K - K // 2)


def test_shared_batch_has_several_batches(oracle):
    assert len(gc.be_events("recon", "shared_batch").col0) == 3 and gc.RECON["shared_batch"]["per_batch"] > 2 * 2048


FE_PACKETS = [("exact", 1.0), ("band", 1.0), ("corners", 1.0), ("last", 1.0), ("band", 0.0), ("corners", 2.0), ("band", 2.0)]


@pytest.mark.parametrize("kind,sigma", FE_PACKETS)
@pytest.mark.parametrize("omega", gc.FE_OMEGAS)
def test_front_end_packets_catch_every_mutation(oracle, kind, sigma, omega):
    p = gc.fe_packet(kind, sigma)
    ev = gc.fe_events(p, omega)
    r = dio.radius(sigma)
    extra = []
    if kind in ("band", "corners") and r > 0:
        corners = gr.corner_events(ev, r)
        assert len(corners) > (0.5 * ev.n if kind == "corners" else 10), (kind, len(corners), ev.n)
        e = int(corners[np.argmax(gr.border_weight(ev, sigma)[corners])])  # (the corner event whose border term is the largest)
        extra.append(("border term skipped at a corner", gr.mutate_skip_s2(ev, e)))
    if kind == "band":
        edge = (ev.xx <= r) | (ev.xx + 1 >= ev.W - 1 - r) | (ev.yy <= r) | (ev.yy + 1 >= ev.H - 1 - r)
        assert edge.mean() > (0.99 if omega == gc.FE_OMEGAS[0] else 0.5) or r == 0, edge.mean()
    if kind == "last" and omega == gc.FE_OMEGAS[0]:
        assert ((ev.xx == 1) | (ev.xx == ev.W - 3) | (ev.yy == 1) | (ev.yy == ev.H - 3)).all() and ev.n == 3000
    mutation_ratios("front end %s sigma %g omega %s" % (kind, sigma, omega), ev, sigma, 0, extra)


@pytest.mark.parametrize("n", gc.FE_COUNTS)
def test_front_end_counts_catch_a_dropped_event(oracle, n):
    p = gc.fe_packet("count", 1.0, n)
    for omega in gc.FE_OMEGAS:
        ev = gc.fe_events(p, omega)
        assert ev.n >= 0.9 * n
        mutation_ratios("front end %d events omega %s" % (n, omega), ev, 1.0, 0)
    ev = gc.fe_events(p, gc.FE_OMEGAS[1])
    mutation_ratios("front end %d events, gradient magnitude" % n, ev, 1.0, 2) if n == 1025 else None


# ------------------------------------------------------------------------------- what the present comparison sees of the same
@pytest.mark.parametrize("name", ["A", "B"])
def test_present_comparison_against_the_same_mutations(oracle, name):
    """cases A and B of recon_cases.py (several batches per knot segment, a knot sees thousands of events): 16 batches spread over the
    stream, in each the event of median weight and the heaviest one moved to the next batch or dropped, and the batch's columns
    shifted -- against rel_vec(g', g) < RTOL, the comparison test_gpu_recon_grad.py makes, and against bound_k.  A report (the counts
    go to profiles/gather_parity.txt); asserted is only that every mutation moves the gradient."""
    c, (w, x, y, t) = rc.CASES[name], rc.window(name)
    ev = gr.be_events(x, y, t, w.lut, rc.SENSOR[0], c["Wp"], c["Hp"], c["order"], rg.point(name), w.start_ns, w.dt_ns, 0, c["batch"],
                      c["rate"])
    Jt, A = host_planes(ev, 1.0, 0)
    ref = gr.gather(ev, Jt, A, 1.0, 0)
    wt = gr.weight(ev, Jt)
    nb = len(ev.col0)
    muts = []
    for b in np.linspace(1, nb - 3, 16).astype(int):
        in_b = np.nonzero(ev.batch == b)[0]
        order = in_b[np.argsort(wt[in_b])]
        for tag, e in (("median event", int(order[len(order) // 2])), ("heaviest event", int(order[-1]))):
            muts.append((tag + " to the next batch", gr.mutate_next_batch(ev, e)))
            muts.append((tag + " dropped", gr.mutate_drop(ev, e)))
        muts.append(("columns shifted", gr.mutate_shift_columns(ev, int(b))))
    missed, caught, total, least = {}, {}, {}, {}
    for kind, mut in muts:
        g = gr.gather_value(mut, Jt, ref.mu, 1.0, 0)
        assert (g != ref.g).any()
        total[kind] = total.get(kind, 0) + 1
        least[kind] = min(least.get(kind, np.inf), rel_vec(g, ref.g))
        missed[kind] = missed.get(kind, 0) + int(rel_vec(g, ref.g) < RTOL)
        caught[kind] = caught.get(kind, 0) + int((np.abs(g - ref.g) > ref.bound).any())
    print("present comparison, case %s (%d events, %d batches, %d parameters), mutations that change rel_vec by less than RTOL = %g "
          "| that exceed bound_k (least change of rel_vec): %s" %
          (name, ev.n, nb, ev.P, RTOL, "; ".join("%s %d | %d of %d (%.1e)" % (k, missed[k], caught[k], total[k], least[k]) for k in total)))
