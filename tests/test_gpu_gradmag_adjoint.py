"""-m gpu: the adjoint gradient of the Sobel gradient-magnitude contrast (contrast_measure = 2) on the production path.

    B = G I, gx = Sx B, gy = Sy B;  contrast = mean(gx^2 + gy^2);  grad_k = (2/N) <D_k, G^T (Sx^T gx + Sy^T gy)>

(tests/test_gradmag_adjoint_identity.py pins the formula on the CPU.)  image_adjoint_sobel_kernel forms Jt per 64 x 16 tile; the
splat, the gather, image reuse, the speculative and the gated pass are the ones variance and mean-square use.  Parity is against
the CPU oracle's eval(measure=2), which computes the gradient from derivative planes as the reference does.  The production side
is the plain hip.FrontendEvaluator -- the library's default -- unless a case says otherwise."""
import functools

import numpy as np
import pytest

from cmax_slam_amd import _lib, synth
from util import RTOL, rel_scalar, rel_vec

pytestmark = pytest.mark.gpu

GRADMAG = 2
OMEGAS = [(0.0, 0.0, 0.0), (0.6, -0.9, 0.4), (-2.0, 1.5, 3.0)]


@functools.lru_cache(maxsize=None)
def _packet(W, H, n):
    if (W, H) == (240, 180):
        return synth.frontend_packet(n, 240, 180, 200.0, 200.0, 119.5, 89.5, seed=11)
    return synth.frontend_packet(n, W, H, 0.83 * max(W, H), 0.83 * max(W, H), (W - 1) / 2.0, (H - 1) / 2.0, seed=7 + W)


def _oracle(oracle, p, measure=GRADMAG, sigma=None, batch=None):
    ref = oracle.Frontend(p.W, p.H, p.lut, p.fx, p.fy, p.cx, p.cy, p.batch if batch is None else batch,
                          p.sigma if sigma is None else sigma, measure)
    ref.set_packet(p.x, p.y, p.t_ns, p.t_ref_ns)
    return ref


def _set(fe, p, measure=GRADMAG, sigma=None, batch=None):
    fe.set_packet(p.x, p.y, p.t_ns, p.t_ref_ns, p.fx, p.fy, p.cx, p.cy, p.batch if batch is None else batch,
                  p.sigma if sigma is None else sigma, measure)


def _pair(hip, oracle, p, sigma=None, batch=None):
    fe = hip.FrontendEvaluator(p.W, p.H, p.lut)
    _set(fe, p, sigma=sigma, batch=batch)
    return fe, _oracle(oracle, p, sigma=sigma, batch=batch)


def _check(tag, got, want):
    c, g = got
    c_ref, g_ref = want
    ec = rel_scalar(c, c_ref)
    eg = rel_vec(g, g_ref) if g is not None else 0.0
    print(f"{tag}: contrast {ec:.2e} gradient {eg:.2e}")
    assert ec < RTOL, tag
    assert eg < RTOL, tag


def _gather_launches(fe, call):
    """Launches of the gather kernel -- the adjoint form's signature -- during call()."""
    fe.timing_enable()
    fe.timing_get()
    out = call()
    n = fe.timing_get()["gather"][1]
    fe.timing_enable(False)
    return out, n


def test_the_adjoint_form_runs(hip, oracle):
    """f then df at one point: the cost-only evaluation leaves Jt behind (speculative image pass), the df reuses it and ends in the
    gather.  With the derivative-plane form all three counters stay 0."""
    p = _packet(240, 180, 30_017)
    fe, ref = _pair(hip, oracle, p)
    om = OMEGAS[1]
    want = ref.eval(om)
    fe.timing_enable()
    fe.timing_get()
    c, _ = fe.eval(om, want_grad=False)
    got = fe.eval(om, want_grad=True)
    s = fe.stats()
    t = fe.timing_get()
    assert s["spec_images"] >= 1
    assert s["reuse_hits"] == 1
    assert t["gather"][1] >= 1
    _check("f", (c, None), want)
    _check("df", got, want)


@pytest.mark.parametrize("W,H,n", [(64, 16, 700), (70, 40, 3_001), (130, 33, 5_000), (23, 19, 257), (240, 180, 30_017)])
def test_tile_shapes(hip, oracle, W, H, n):
    """One tile exactly (every halo a reflection), partial tiles on both axes, remainders of 2 columns and 1 row (a halo that crosses
    a tile seam and the border together), an image smaller than a tile, many tiles: fdf, df alone, f alone."""
    p = _packet(W, H, n)
    fe, ref = _pair(hip, oracle, p)
    want = [ref.eval(om) for om in OMEGAS]
    for om, w in zip(OMEGAS, want):
        f, df = fe.contrast_fdf(om)
        _check(f"{W}x{H} fdf {om}", (-f, -df), w)
    for om, w in zip(OMEGAS, want):  # (the point before it is another one: a fresh evaluation, no resident image)
        _check(f"{W}x{H} df {om}", (w[0], -fe.contrast_df(om)), w)
    for om, w in zip(OMEGAS, want):
        _check(f"{W}x{H} f {om}", (-fe.contrast_f(om), None), w)


@pytest.mark.parametrize("sigma,batch", [(0.0, 100), (0.5, 100), (2.0, 64), (1.0, 1)])
def test_blur_and_batch(hip, oracle, sigma, batch):
    """Radius 0 (Jt = (Sx^T Sx + Sy^T Sy) I), 2, 8 through the generic-radius kernel, 4 through the unrolled one."""
    p = _packet(70, 40, 3_001)
    fe, ref = _pair(hip, oracle, p, sigma=sigma, batch=batch)
    for om in OMEGAS:
        want = ref.eval(om)
        (got, launches) = _gather_launches(fe, lambda: fe.eval(om))
        assert launches >= 1
        _check(f"sigma {sigma} batch {batch} {om}", got, want)
        _check(f"sigma {sigma} batch {batch} f {om}", fe.eval(om, want_grad=False), want)


@pytest.mark.parametrize("W,H,adjoint", [(9, 24, False), (24, 9, False), (10, 10, True)])
def test_both_sides_of_the_size_rule(hip, oracle, W, H, adjoint):
    """adjoint_ok(): each side > 2r + 1 (the G^T folds; Sobel^T needs a side of 2 only).  sigma = 1 -> r = 4: a side of 9 keeps the
    derivative-plane form, 10 x 10 is the smallest image that takes the adjoint form."""
    p = _packet(W, H, 400)
    fe, ref = _pair(hip, oracle, p)
    for om in OMEGAS:
        want = ref.eval(om)
        (got, launches) = _gather_launches(fe, lambda: fe.eval(om))
        assert (launches >= 1) == adjoint
        _check(f"{W}x{H} {om}", got, want)
        _check(f"{W}x{H} f {om}", fe.eval(om, want_grad=False), want)


def test_sparse_scene_and_pingpong_upkeep(hip, oracle):
    """Votes in one corner, next to tile seams; most tiles empty.  Consecutive evaluations alternate the two vote buffers, each
    image pass clearing the other: a pass that forgets it, or looks too short a way for votes, shows here."""
    full = _packet(240, 180, 30_017)
    keep = (full.x < 70) & (full.y < 40)
    p = synth.FrontendPacket(full.W, full.H, full.fx, full.fy, full.cx, full.cy, full.x[keep], full.y[keep], full.t_ns[keep],
                             full.t_ref_ns, full.omega_true)
    assert 500 < len(p.x) < len(full.x) // 4
    fe, ref = _pair(hip, oracle, p)
    seq = [((0.6, -0.9, 0.4), True), ((-2.0, 1.5, 3.0), True), ((4.0, -3.0, 5.0), False), ((0.0, 0.0, 0.0), True)]
    for i, (om, want_grad) in enumerate(seq):
        _check(f"sparse {i} {om}", fe.eval(om, want_grad=want_grad), ref.eval(om))


def test_measure_switching_on_one_context(hip, oracle):
    """Variance, gradient magnitude, mean-square, gradient magnitude on ONE context: no stale Jt or moment rows, the right image
    pass each time."""
    p = _packet(70, 40, 3_001)
    fe = hip.FrontendEvaluator(p.W, p.H, p.lut)
    om = OMEGAS[1]
    for measure in (0, 2, 1, 2):
        _set(fe, p, measure=measure)
        want = _oracle(oracle, p, measure=measure).eval(om)
        _check(f"measure {measure} f", fe.eval(om, want_grad=False), want)
        _check(f"measure {measure} df", fe.eval(om), want)
        _check(f"measure {measure} fdf", fe.eval(OMEGAS[2]), _oracle(oracle, p, measure=measure).eval(OMEGAS[2]))


def test_gated_pass(hip, oracle):
    p = _packet(240, 180, 30_017)
    fe, ref = _pair(hip, oracle, p)
    om = OMEGAS[1]
    want = ref.eval(om)
    before = fe.stats()["gated_hits"]
    fe.hint_next_df(0.0, 4)
    _check("gated f", fe.eval(om, want_grad=False), want)
    _check("gated df", fe.eval(om), want)
    assert fe.stats()["gated_hits"] - before == 1


@pytest.mark.parametrize("want_grad", [True, False])
def test_eval_many(hip, oracle, want_grad):
    p = _packet(70, 40, 3_001)
    fe, ref = _pair(hip, oracle, p)
    pts = OMEGAS + [(0.3, -0.5, 0.2)]
    cs, gs = fe.eval_many(pts, want_grad=want_grad)
    for i, om in enumerate(pts):
        want = ref.eval(om)
        _check(f"eval_many {i}", (cs[i], gs[i] if want_grad else None), want)
        _check(f"eval {i}", fe.eval(om, want_grad=want_grad), want)


def test_deterministic_mode(hip, oracle):
    p = _packet(130, 33, 5_000)
    ref = _oracle(oracle, p)
    om = OMEGAS[1]
    got = []
    for _ in range(2):
        fe = hip.FrontendEvaluator(p.W, p.H, p.lut)
        fe.set_option(_lib.OPT_DETERMINISTIC, 1)
        _set(fe, p)
        (r, launches) = _gather_launches(fe, lambda: fe.eval(om))
        assert launches >= 1
        got.append(r)
        fe.close()
    assert got[0][0] == got[1][0]
    assert np.array_equal(got[0][1], got[1][1])
    _check("deterministic", got[0], ref.eval(om))


def test_split_phase(hip, oracle):
    p = _packet(130, 33, 5_000)
    fe, ref = _pair(hip, oracle, p)
    om = OMEGAS[2]
    want = ref.eval(om)
    fe.accumulate(om, True)
    fe.finish_begin(True)
    got = fe.finish_end(True)
    _check("split", got, want)
    _check("eval", fe.eval(om), want)
    fe.accumulate(om, False)
    fe.finish_begin(False)
    _check("split f", fe.finish_end(False), want)


def test_solve(hip, oracle):
    """FR-CG from zero on the production context and on the reference-shaped one: both stop by the driver's tolfun = 1e-4, so the
    contrasts they reach may differ by that much.  The device-driven solve stays out of it (chain_eligible)."""
    p = _packet(240, 180, 30_017)
    ref = _oracle(oracle, p)
    fe = hip.FrontendEvaluator(p.W, p.H, p.lut)
    _set(fe, p)
    x_prod, rep_prod = fe.setupProblemAndOptimize((0.0, 0.0, 0.0))
    assert fe.stats()["chain_solves"] == 0
    fr = hip.reference_shaped.FrontendEvaluator(p.W, p.H, p.lut)
    _set(fr, p)
    x_ref, rep_ref = fr.setupProblemAndOptimize((0.0, 0.0, 0.0))
    c_prod, c_ref = ref.eval(x_prod, want_grad=False)[0], ref.eval(x_ref, want_grad=False)[0]
    print(f"solve: production {x_prod} -> {c_prod!r} {rep_prod}\n       reference-shaped {x_ref} -> {c_ref!r} {rep_ref}")
    assert c_prod >= c_ref * (1.0 - 1e-4)
