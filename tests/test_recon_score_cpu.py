"""CPU: the references of the per-event support score tests (tests/recon_score_cases.py) checked on their own, before a device is
compared with them, and the declarations the feature adds.

(a) sum identity.  With sigma 0 and no leave-one-out, sum_{flags == 3} score_i = sum_i sum_c w_ic P[c] = sum_c P[c] sum_i w_ic = sum P^2
    when P is the sum of the votes.  Checked in fp64 to 1e-12 relative on the plane the reference coordinates vote in fp64 (plane64) --
    the oracle's own plane is an fp32 accumulation of the same votes, so on it the identity holds to fp32 rounding only; plane64 is
    tied to the oracle plane within the tolerance tests/test_gpu_recon.py uses (util.RTOL).
(b) the closed form of the own contribution equals w^T (Gy (x) Gx) w from the dense operators on every event of the border cases.
(c) the border cases hit the borders: at least MIN_FOLDED voting events with a folded tap at each of the four, for sigma 1 and 2."""
import os
import re

import numpy as np
import pytest

import recon_score_cases as sc
import recon_warp_cases as wc
from util import RTOL, rel_img

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ("cmx_backend_recon_score_open", "cmx_backend_recon_score_plane", "cmx_backend_recon_score", "cmx_backend_recon_score_aos",
         "cmx_backend_recon_score_from", "cmx_backend_recon_score_from_device")
NAMES = ("A", "B", "poles") + tuple(sc.BORDER)


def test_header_and_binding_declare_the_calls():
    from cmax_slam_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "cmax_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in CALLS:
        assert re.search(r"\bint\s+%s\s*\(" % name, code), name
        assert name in _lib.SYMBOLS
    assert re.search(r"#define\s+CMX_ABI_VERSION\s+6\b", hdr)  # symbols only: the ABI version stays
    from cmax_slam_amd import evaluator
    for m in ("reconstruct_score_open", "reconstruct_score_plane", "reconstruct_score", "reconstruct_score_aos", "reconstruct_score_from"):
        assert callable(getattr(evaluator.BackendEvaluator, m))


@pytest.mark.parametrize("name", NAMES)
def test_sum_identity_on_the_reference(oracle, name):
    c = sc.case(name)[0]
    px, py, fl = sc.reference(name)
    P = sc.plane64(px, py, fl, c["Hp"], c["Wp"])
    r = rel_img(P, sc.oracle_plane(name))
    m = fl == 3
    xx, yy, dx, dy = sc.cells(px[m], py[m])
    w = sc.iwe_numpy._weights(dx, dy).astype(np.float64)
    score = ((w[:, 0] * P[yy, xx] + w[:, 1] * P[yy, xx + 1]) + w[:, 2] * P[yy + 1, xx]) + w[:, 3] * P[yy + 1, xx + 1]
    lhs, rhs = float(score.sum()), float((P * P).sum())
    print("%s: %d voting events, sum score %.12e, sum P^2 %.12e, rel %.2e; plane64 vs the oracle plane %.2e" %
          (name, int(m.sum()), lhs, rhs, abs(lhs - rhs) / rhs, r))
    assert m.sum() > 1000 and rhs > 0
    assert abs(lhs - rhs) <= 1e-12 * rhs
    assert r < RTOL
    # the fp32 emulation on the fp32 image of that plane is the same sum up to its seven roundings per term
    s32 = sc.score32(P.astype(np.float32), px, py, fl)
    assert abs(float(s32[m].sum(dtype=np.float64)) - rhs) <= 2.0 ** -20 * rhs
    assert (s32[(fl & wc.INSIDE) == 0] == 0).all()


@pytest.mark.parametrize("sigma", sc.SIGMAS)
@pytest.mark.parametrize("name", tuple(sc.BORDER))
def test_closed_form_self_term_equals_the_dense_operators(oracle, name, sigma):
    c = sc.case(name)[0]
    px, py, fl = sc.reference(name)
    m = (fl & wc.INSIDE) != 0
    closed, fold = sc.self_closed(px[m], py[m], c["Hp"], c["Wp"], sigma)
    dense = sc.self_ref(px[m], py[m], c["Hp"], c["Wp"], sigma, exact_products=True)
    err = float(np.abs(closed / dense - 1).max())
    print("%s sigma %g: %d events, %d with a folded tap, max relative difference %.2e" % (name, sigma, int(m.sum()), int(fold.any(axis=1).sum()), err))
    assert (dense > 0).all() and err <= 1e-13
    # the fp32 vote weights instead of the exact products: what the event really added; two roundings apart
    voted = sc.self_ref(px[m], py[m], c["Hp"], c["Wp"], sigma)
    assert float(np.abs(voted / dense - 1).max()) <= 4 * 2.0 ** -24
    # an event away from the borders has the interior value, whatever its cell
    taps = sc.taps_of(sigma)
    r = (len(taps) - 1) // 2
    xx, yy, dx, dy = sc.cells(px[m], py[m])
    ux, uy = (np.float32(1) - dx).astype(np.float64), (np.float32(1) - dy).astype(np.float64)
    vx, vy = dx.astype(np.float64), dy.astype(np.float64)
    interior = ((ux * ux + vx * vx) * taps[r] + 2 * ux * vx * taps[r + 1]) * ((uy * uy + vy * vy) * taps[r] + 2 * uy * vy * taps[r + 1])
    free = ~fold.any(axis=1)
    assert free.sum() > 1000 and float(np.abs(closed[free] / interior[free] - 1).max()) <= 1e-13
    assert float(np.abs(closed[~free] / interior[~free] - 1).max()) > 1e-3  # (and the folds matter where they occur)


@pytest.mark.parametrize("name", tuple(sc.BORDER))
def test_border_cases_hit_all_four_borders(oracle, name):
    c = sc.case(name)[0]
    px, py, fl = sc.reference(name)
    assert np.count_nonzero(wc.near_integer(px, py)) <= wc.MAX_NEAR_INTEGER
    xx, yy = sc.cells(px[fl == 3], py[fl == 3])[:2]
    for sigma in sc.SIGMAS:
        r = (len(sc.taps_of(sigma)) - 1) // 2
        assert c["Wp"] > 2 * r + 1 and c["Hp"] > 2 * r + 1
        n = sc.events_with_fold(name, sigma)
        print("%s sigma %g (r %d): voting events with a folded tap at the left / right / top / bottom border: %s" % (name, sigma, r, n))
        assert (n >= sc.MIN_FOLDED).all()
        # votes on both sides of the seam and at both poles, within the radius
        assert (xx <= r - 1).sum() >= sc.MIN_FOLDED and (xx + 1 >= c["Wp"] - r).sum() >= sc.MIN_FOLDED
        assert (yy <= r - 1).sum() >= sc.MIN_FOLDED and (yy + 1 >= c["Hp"] - r).sum() >= sc.MIN_FOLDED


def test_leave_one_out_of_a_lone_event_is_zero():
    """an event alone in its four cells: S = its own weights, score == self bit for bit"""
    px, py = np.array([17.3, 100.75]), np.array([40.6, 9.125])
    fl = np.array([3, 3], np.uint8)
    S = sc.plane64(px, py, fl, 64, 128).astype(np.float32)
    s = sc.score32(S, px, py, fl)
    assert (s > 0).all() and (sc.loo32(s, sc.self0_32(px, py), fl) == 0).all()
    assert (sc.loo32(s, sc.self0_32(px, py), np.array([2, 1], np.uint8)) == s).all()
