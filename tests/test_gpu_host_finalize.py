"""-m gpu: the host finalize of front-end gradient evaluations (CMX_OPT_TAIL_FINALIZE = 4, cmx_hostfin.hpp) against the device tail
(value 1) it replaces.

How the two forms are compared.  Two fresh evaluations of one point differ in the last bits of the IMAGE (order of the fp32 vote
atomics), so a fresh value-4 evaluation cannot be held to a fresh value-1 one bit for bit.  A repeated evaluation of the point the
context has just evaluated reuses the resident planes (CMX_OPT_REUSE_IMAGE, the library's default): the image pass is deterministic
on given planes, so both evaluations read the SAME moment rows and the same Jt, and what is left to differ is the end of the gather
launch -- exactly what the option changes.  Every comparison below is such a pair on one context, in both orders (value 1 first,
value 4 fresh first); the gradient's noise bound is applied between two evaluations on resident planes, one of each form.
* contrast: the same two moment sums in the same order of additions through the same expression -> bit-identical.
* gradient: the gather's fp64 atomic adds to the accumulator rows land in an order that varies run to run.  The test measures that
  noise itself -- the largest max-norm relative difference between any two of SAMPLES value-1 evaluations of the same point,
  printed -- and holds value 4 to twice it.  Where every accumulator row receives at most two sums (G <= 16) the
  order cannot matter, the measured noise is 0 and the gradients must agree bit for bit (shard count 8: the same rows summed in the
  same order).
* both within 1e-5 of the CPU oracle, the project's bound.
"""
import numpy as np
import pytest

from cmax_slam_amd import _lib, synth
from util import RTOL, rel_scalar, rel_vec

pytestmark = pytest.mark.gpu

SAMPLES = 160  # value-1 evaluations per case (30 us each): every two of them are a pair, 12 720 pairs (at least 20 are asked for).  The
               # differences are one or two units in the last place of one component, and which component moves is rare luck: over 40
               # consecutive pairs the largest seen was one unit of a small component (1.5e-16 of the max-norm) where a value-4
               # result then sat one unit of the largest component (3.1e-16) from a value-1 one -- the largest difference of a few
               # pairs underestimates what two evaluations can show, so the test takes enough of them to have seen it
# events -> workgroups of the gather (fe_gather_blocks): 2 (shards without a member), 8 (one workgroup per shard), 9 (one shard of
# two), 235 (many per shard)
EVENTS = {300: 2, 2048: 8, 2304: 9, 60_000: 235}
OM = np.array([0.3, -0.5, 0.2])
WRONG_RECORD = 1e-9   # gradient difference (max-norm relative) beyond which two results are not the same evaluation's: neighbouring
                      # points of these tests are 2e-2 or more apart, reordered fp64 sums 1e-15
_packets, _refs = {}, {}


def _packet(W, H, n):
    if (W, H, n) not in _packets:
        _packets[(W, H, n)] = synth.frontend_packet(n, W, H, 0.9 * W, 0.9 * W, (W - 1) / 2, (H - 1) / 2, seed=W + H + n)
    return _packets[(W, H, n)]


def _oracle_at(oracle, p, measure, om):
    """(contrast, gradient) of the CPU oracle, computed once per (packet, measure, point) and shared"""
    key = (p.W, p.H, len(p.x), measure, tuple(np.round(om, 12)))
    if key not in _refs:
        ref = oracle.Frontend(p.W, p.H, p.lut, p.fx, p.fy, p.cx, p.cy, p.batch, p.sigma, measure)
        ref.set_packet(p.x, p.y, p.t_ns, p.t_ref_ns)
        _refs[key] = ref.eval(om)
    return _refs[key]


def _fe(hip, p, measure, fused=1, tail=None):
    fe = hip.FrontendEvaluator(p.W, p.H, p.lut)
    fe.set_option(_lib.OPT_FUSED_IMAGE, int(fused))
    if tail is not None:
        fe.set_option(_lib.OPT_TAIL_FINALIZE, tail)
    fe.set_packet(p.x, p.y, p.t_ns, p.t_ref_ns, p.fx, p.fy, p.cx, p.cy, p.batch, p.sigma, measure)
    return fe


def _bits(v):
    return np.asarray(v, np.float64).view(np.uint64)


def _host_evals(fe):
    return fe.stats()["host_finalize_evals"]


def _eval_as(fe, tail, om):
    """one gradient evaluation under option value `tail`; (contrast, gradient, evaluations the host finalized in it)"""
    fe.set_option(_lib.OPT_TAIL_FINALIZE, tail)
    before = _host_evals(fe)
    c, g = fe.eval(om)
    return c, np.array(g), _host_evals(fe) - before


def _pair_noise(fe, om, samples):
    """`samples` value-1 evaluations of `om` (after the first the resident image is reused): the largest gradient difference that any
    two of them show -- samples * (samples - 1) / 2 pairs --, their contrast, the last gradient"""
    c0, g, k = _eval_as(fe, 1, om)
    assert k == 0
    gs = [g]
    for _ in range(samples - 1):
        c, g, k = _eval_as(fe, 1, om)
        assert k == 0 and _bits(c) == _bits(c0)   # (the premise: same planes, same moments)
        gs.append(g)
    gs = np.array(gs)
    diff = np.abs(gs[:, None, :] - gs[None, :, :]).max(axis=2) / np.abs(gs).max(axis=1)[None, :]   # rel_vec of every ordered pair
    return float(diff.max()), c0, gs[-1]


@pytest.mark.parametrize("fused", [1, 0])
@pytest.mark.parametrize("measure", [0, 1])
@pytest.mark.parametrize("n", sorted(EVENTS))
@pytest.mark.parametrize("W,H", [(64, 48), (100, 70), (346, 260)])
def test_host_finalize_equals_device_tail(hip, oracle, W, H, n, measure, fused):
    p = _packet(W, H, n)
    fe = _fe(hip, p, measure, fused)
    cr, gr = _oracle_at(oracle, p, measure, OM)
    # value 1 first, value 4 on the same planes
    noise, c1, g1 = _pair_noise(fe, OM, SAMPLES)
    assert fe.stats()["events"] == n
    worst = 0.0
    for _ in range(6):
        c4, g4, k = _eval_as(fe, 4, OM)
        assert k == 1, "the evaluation did not take the host finalize"
        assert _bits(c4) == _bits(c1), (c4, c1)
        worst = max(worst, rel_vec(g4, g1))
        assert rel_scalar(c4, cr) < RTOL and rel_vec(g4, gr) < RTOL, (c4, cr, g4, gr)
    print("host_finalize %dx%d n %d (G %d) measure %d fused %d: value-1 pair noise over %d pairs %.3e, value 4 vs value 1 %.3e (bound %.3e)"
          % (W, H, n, EVENTS[n], measure, fused, SAMPLES * (SAMPLES - 1) // 2, noise, worst, 2.0 * noise))
    assert worst <= 2.0 * noise, (worst, noise)
    # value 4 on a FRESH image (the whole evaluation: splat, image pass, gather, records), then value 1 on its planes.  A gather that
    # starts behind a splat does not see its workgroups finish in the order a gather on resident planes does, so this pair is not one
    # the measured noise describes: the contrast must be the same bits, both gradients the oracle's, and the two gradients the
    # same evaluation's (WRONG_RECORD: far above any reordering of 235 fp64 adds, far below what another evaluation's sums would do)
    om2 = OM + np.array([0.02, -0.01, 0.015])
    cr2, gr2 = _oracle_at(oracle, p, measure, om2)
    c4, g4, k = _eval_as(fe, 4, om2)
    assert k >= 1
    c1b, g1b, k = _eval_as(fe, 1, om2)
    assert k == 0 and _bits(c4) == _bits(c1b), (c4, c1b)
    assert rel_vec(g4, g1b) < WRONG_RECORD, (g4, g1b)
    assert rel_scalar(c4, cr2) < RTOL and rel_vec(g4, gr2) < RTOL and rel_vec(g1b, gr2) < RTOL, (c4, cr2, g4, gr2)


def test_300_evaluations_cycling_through_8_points(hip, oracle):
    """Tickets advance by one per evaluation and every record line is rewritten 300 times: an accepted record of an earlier
    evaluation would carry another point's sums (the 8 points' gradients differ by far more than the bound)."""
    p = _packet(100, 70, 60_000)
    fe = _fe(hip, p, 0)
    rng = np.random.default_rng(8)
    pts = [OM + rng.normal(0, 0.05, 3) for _ in range(8)]
    noise = max(_pair_noise(fe, om, 40)[0] for om in pts)   # 8 x 780 pairs
    grads = np.array([_eval_as(fe, 1, om)[1] for om in pts])
    sep = min(rel_vec(grads[i], grads[j]) for i in range(8) for j in range(i))
    assert sep > 1e3 * max(noise, 1e-16), (sep, noise)
    worst, finalized = 0.0, 0
    for i in range(300):
        om = pts[i % 8]
        first, second = (4, 1) if i % 2 else (1, 4)
        ca, ga, ka = _eval_as(fe, first, om)    # a fresh image
        cb, gb, kb = _eval_as(fe, second, om)   # the other form on its planes
        cc, gc, kc = _eval_as(fe, first, om)    # ... and the first form again, like for like with the second
        assert ka + kb == 1 and kc == ka, (i, ka, kb, kc)
        finalized += ka
        finalized += kb
        assert _bits(ca) == _bits(cb) == _bits(cc), (i, ca, cb, cc)
        assert rel_vec(ga, gb) < WRONG_RECORD, (i, ga, gb)
        worst = max(worst, rel_vec(gb, gc))
        assert rel_vec(gb, gc) <= 2.0 * noise, (i, gb, gc, noise)
    assert finalized == 300
    for om, g in zip(pts, grads):
        cr, gr = _oracle_at(oracle, p, 0, om)
        c4, g4, _ = _eval_as(fe, 4, om)
        assert rel_scalar(c4, cr) < RTOL and rel_vec(g4, gr) < RTOL
    print("host_finalize cycle: 300 evaluations, value-1 pair noise %.3e (8 x 780 pairs), worst value 4 vs value 1 %.3e, points apart by %.3e"
          % (noise, worst, sep))


def test_jump_beyond_the_tiles_reach_is_repeated(hip, oracle):
    """The fallback word travels in the moments record: a jump of omega far beyond the tiles' reach must be noticed by the host,
    the evaluation repeated after a fresh sort, and the result right."""
    p = synth.frontend_packet(60_013, 240, 180, 200.0, 200.0, 119.5, 89.5, seed=21)
    fe = _fe(hip, p, 0, fused=1, tail=4)
    seq = [(0.0, 0.0, 0.0), (6.0, -5.0, 9.0), (6.02, -5.0, 9.0), (-4.0, 3.0, -8.0), (0.0, 0.0, 0.0)]
    redos = 0
    for om in seq:
        before = fe.stats()
        c, g = fe.eval(om)
        after = fe.stats()
        cr, gr = _oracle_at(oracle, p, 0, np.array(om))
        assert rel_scalar(c, cr) < RTOL and rel_vec(g, gr) < RTOL, (om, c, cr, g, gr)
        d = after["fused_redos"] - before["fused_redos"]
        assert after["host_finalize_evals"] - before["host_finalize_evals"] == 1 + d, (om, before, after)
        redos += d
    s = fe.stats()
    assert redos >= 2 and s["fused_redos"] >= 2 and s["rebins"] >= 3, s


@pytest.mark.parametrize("spin", [0, 2])
def test_stream_synchronize_path(hip, oracle, spin):
    """CMX_OPT_SPIN_WAIT 0: no spinning, the host blocks in hipStreamSynchronize and must then find every record; 2: a spin budget of
    2 us, which an evaluation outlasts -- the spin gives up with some records taken and the rest follow after the synchronisation.
    The library's default for CMX_OPT_TAIL_FINALIZE is left alone: eligible evaluations take the host finalize unasked."""
    p = _packet(100, 70, 60_000)
    fe = hip.FrontendEvaluator(p.W, p.H, p.lut)
    fe.set_option(_lib.OPT_SPIN_WAIT, spin)
    fe.set_packet(p.x, p.y, p.t_ns, p.t_ref_ns, p.fx, p.fy, p.cx, p.cy, p.batch, p.sigma, 0)
    rng = np.random.default_rng(17)
    for i in range(12):
        om = OM + rng.normal(0, 0.05, 3)
        before = _host_evals(fe)
        c, g = fe.eval(om)
        assert _host_evals(fe) == before + 1, "the default did not take the host finalize"
        cr, gr = _oracle_at(oracle, p, 0, om)
        assert rel_scalar(c, cr) < RTOL and rel_vec(g, gr) < RTOL, (i, c, cr, g, gr)
        c1, g1, k = _eval_as(fe, 1, om)   # the device tail on the same planes
        assert k == 0 and _bits(c1) == _bits(c), (i, c1, c)
        assert rel_vec(g1, gr) < RTOL
        fe.set_option(_lib.OPT_TAIL_FINALIZE, 4)


def test_other_entry_points_keep_the_device_finalize(hip, oracle):
    """eval_many and device-driven solves on a context with value 4 set: they are not eligible, and give what value 1 gives.  (Fresh
    evaluations on two settings: the planes differ by the order of the fp32 vote atomics -- the bounds are those
    tests/test_gpu_fused.py holds two forms of a fresh evaluation to, 1e-7 / 1e-6, and the oracle's 1e-5.)"""
    p = _packet(100, 70, 60_000)
    fe = _fe(hip, p, 0)
    rng = np.random.default_rng(3)
    xs = OM + rng.normal(0, 0.05, (6, 3))
    fe.set_option(_lib.OPT_TAIL_FINALIZE, 1)
    c1, g1 = fe.eval_many(xs)
    fe.set_option(_lib.OPT_TAIL_FINALIZE, 4)
    before = _host_evals(fe)
    c4, g4 = fe.eval_many(xs)
    assert _host_evals(fe) == before
    for i in range(len(xs)):
        cr, gr = _oracle_at(oracle, p, 0, xs[i])
        assert rel_scalar(c4[i], c1[i]) < 1e-7 and rel_vec(g4[i], g1[i]) < 1e-6, (i, c4[i], c1[i])
        assert rel_scalar(c4[i], cr) < RTOL and rel_vec(g4[i], gr) < RTOL
    # cost-only evaluations and the gated pass behind them (conjugate_fr's f, then df at the same point)
    om = xs[0]
    cr, gr = _oracle_at(oracle, p, 0, om)
    fe.hint_next_df(0.0, 4)
    assert rel_scalar(-fe.contrast_f(om), cr) < RTOL
    assert rel_vec(-fe.contrast_df(om), gr) < RTOL
    # a device-driven solve on each setting
    sol = {}
    for tail in (1, 4):
        q = synth.frontend_packet(100_000, 240, 180, 0.9 * 240, 0.9 * 240, 119.5, 89.5, seed=77)
        s = hip.FrontendEvaluator(q.W, q.H, q.lut)
        s.set_fast_path()
        s.set_option(_lib.OPT_CHAIN_SOLVE, 1)
        s.set_option(_lib.OPT_TAIL_FINALIZE, tail)
        s.set_packet(q.x, q.y, q.t_ns, q.t_ref_ns, q.fx, q.fy, q.cx, q.cy, q.batch, q.sigma, _lib.VARIANCE)
        sol[tail] = s.setupProblemAndOptimize(np.zeros(3))
        st = s.stats()
        assert st["chain_solves"] == 1 and st["chain_takeovers"] == 0, st
    (xa, ra), (xb, rb) = sol[4], sol[1]
    # (two solves of one packet: the closeness tests/test_gpu_chain_solve.py holds two drivers to)
    assert abs(ra["final_cost"] - rb["final_cost"]) < 5e-2 * abs(rb["final_cost"]) and np.abs(xa - xb).max() < 0.2, (sol[4], sol[1])
    assert ra["initial_cost"] == pytest.approx(rb["initial_cost"], rel=1e-6)
    assert ra["final_cost"] <= ra["initial_cost"]
