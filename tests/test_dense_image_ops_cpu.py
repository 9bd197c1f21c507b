"""CPU: the fp64 operators of tests/dense_image_ops.py -- the reference side of tests/test_gpu_adjoint_plane.py -- against the oracle.

Poisson planes (non-negative integers, like a vote image) at sides from the least the adjoint form allows (2r + 2) to 130 x 34 (three
tile columns and rows, one-pixel remainders), radii 2 to 12.  The fp32 comparisons take the bound the GPU test takes
(8 max(e32, 2^-24) of the plane's maximum, e32 the reference's own fp32 pass-by-pass error) with the oracle's fp32 result in the
device's place; everything else is fp64 against fp64.
"""
import numpy as np
import pytest

import dense_image_ops as dio
from util import RTOL, rel_scalar

# (W, H, sigma): radius 2, 4, 7, 8, 12
CASES = [(10, 10, 0.5), (10, 10, 1.0), (64, 16, 1.0), (65, 17, 1.0), (128, 32, 1.0), (100, 70, 1.0), (16, 16, 1.7), (65, 16, 1.7),
         (18, 18, 2.0), (130, 34, 2.0), (26, 26, 3.0), (130, 34, 3.0)]
RADII = {0.5: 2, 1.0: 4, 1.7: 7, 2.0: 8, 3.0: 12}


def poisson_plane(W, H, seed=0):
    return np.random.default_rng(100 * W + H + seed).poisson(3.0, (H, W)).astype(np.float32)


def test_radii(oracle):
    for sigma, r in RADII.items():
        assert dio.radius(sigma) == r
    assert dio.radius(0.0) == 0 and dio.jt_reach(1.0, oracle.GRADIENT_MAGNITUDE) == 10 and dio.jt_reach(1.0, oracle.VARIANCE) == 8


@pytest.mark.parametrize("W,H,sigma", CASES)
def test_blur_matrix_is_the_oracles_blur(oracle, W, H, sigma):
    A = poisson_plane(W, H)
    taps = oracle.gauss_kernel(sigma)
    Gy, Gx = dio.blur_matrix(H, taps), dio.blur_matrix(W, taps)
    B = Gy @ A.astype(np.float64) @ Gx.T
    assert np.abs(B - dio.blurred(A, sigma)).max() <= 1e-14 * np.abs(B).max()
    # the reference side's own fp32 error of the two forward passes -> the bound
    g32y, g32x = dio.Banded.from_filter(H, taps, np.float32), dio.Banded.from_filter(W, taps, np.float32)
    B32 = dio.apply2(g32y, g32x, A)
    assert B32.dtype == np.float32
    scale = np.abs(B).max()
    e32 = np.abs(B32 - B).max() / scale
    err = np.abs(oracle.gaussian_blur(A, sigma).astype(np.float64) - B).max() / scale
    print("blur %dx%d sigma %g: oracle vs dense %.3e of max, e32 %.3e, bound %.3e" % (W, H, sigma, err, e32, 8 * max(e32, dio.EPS32)))
    assert err <= 8 * max(e32, dio.EPS32), (err, e32)
    # every row of a REFLECT_101 blur sums to the taps' sum; the column sums differ from it only within 2r of a border
    # (the mirrored taps of the first r rows land on columns 1 .. r)
    for M, L in ((Gy, H), (Gx, W)):
        assert np.allclose(M.sum(axis=1), taps.astype(np.float64).sum(), rtol=0, atol=1e-15)
        r = RADII[sigma]
        assert np.allclose(M.sum(axis=0)[2 * r:L - 2 * r], taps.astype(np.float64).sum(), rtol=0, atol=1e-15)


@pytest.mark.parametrize("L,r", [(10, 2), (10, 4), (65, 4), (130, 12), (26, 12), (600, 8), (2048, 12)])
def test_banded_form_is_the_dense_matrix_and_transposes(L, r):
    rng = np.random.default_rng(L + r)
    taps = rng.random(2 * r + 1).astype(np.float32)
    Bd = dio.blur_matrix(L, taps, banded=True)
    M = dio.blur_matrix(L, taps, banded=False)
    assert isinstance(Bd, dio.Banded) and isinstance(M, np.ndarray)
    assert isinstance(dio.blur_matrix(L, taps), dio.Banded) == (L > dio.DENSE_MAX)
    assert np.array_equal(Bd.dense(), M) and np.array_equal(Bd.T.dense(), M.T)
    # the matrix, built entry by entry from the definition
    ref = np.zeros((L, L))
    for i in range(L):
        for k in range(2 * r + 1):
            ref[i, dio.reflect101(np.array([i - r + k]), L)[0]] += float(taps[k])
    assert np.array_equal(M, ref)
    a, b = rng.standard_normal((L, 7)), rng.standard_normal((L, 7))
    assert np.abs(Bd.dot(a) - M @ a).max() <= 1e-13 * np.abs(M @ a).max()
    assert np.abs(Bd.T.dot(b) - M.T @ b).max() <= 1e-13 * np.abs(M.T @ b).max()
    for G, Gt in ((M, M.T), (Bd, Bd.T)):   # <G a, b> = <a, G^T b>
        lhs, rhs = np.sum(dio._dot(G, a) * b), np.sum(a * dio._dot(Gt, b))
        assert abs(lhs - rhs) <= 1e-13 * max(abs(lhs), np.sum(np.abs(dio._dot(G, a) * b))), (lhs, rhs)


@pytest.mark.parametrize("W,H,sigma", CASES)
@pytest.mark.parametrize("measure", [0, 2])
def test_jt_is_the_adjoint_of_the_forward_operator(oracle, W, H, sigma, measure):
    """<F a, F b> = <a, Jt(b)> for F = G (measures 0 / 1) and F = (Sx G, Sy G) (measure 2), on random fp64 planes, to 1e-13"""
    rng = np.random.default_rng(W * H + measure)
    a, b = rng.standard_normal((H, W)), rng.standard_normal((H, W))
    Fa, Fb = dio.blurred(a, sigma), dio.blurred(b, sigma)
    if measure == 2:
        Sy, Dy = dio.sobel_matrices(H)
        Sx, Dx = dio.sobel_matrices(W)
        lhs = np.sum((Sy @ Fa @ Dx.T) * (Sy @ Fb @ Dx.T)) + np.sum((Dy @ Fa @ Sx.T) * (Dy @ Fb @ Sx.T))
    else:
        lhs = np.sum(Fa * Fb)
    J = dio.jt_ref(b, sigma, measure)
    rhs = np.sum(a * J)
    assert abs(lhs - rhs) <= 1e-13 * np.sum(np.abs(a * J)), (lhs, rhs)


@pytest.mark.parametrize("W,H", [(10, 10), (65, 17), (130, 34), (2, 2), (3, 2)])
def test_sobel_matrices_are_the_oracles_sobel(oracle, W, H):
    """contrast 2 of a plane = mean (Sx B)^2 + (Sy B)^2.  On small integers every fp32 operation of the oracle is exact."""
    B = poisson_plane(W, H, seed=1)
    Sy, Dy = dio.sobel_matrices(H)
    Sx, Dx = dio.sobel_matrices(W)
    B64 = B.astype(np.float64)
    gx, gy = Sy @ B64 @ Dx.T, Dy @ B64 @ Sx.T
    c = float(np.mean(gx * gx + gy * gy))
    c_or, _ = oracle.contrast(B, None, oracle.GRADIENT_MAGNITUDE, want_grad=False)
    assert c > 0 or min(W, H) <= 2
    assert abs(c - c_or) <= 1e-12 * max(c, 1e-300), (c, c_or)
    # ... and through the blur, where the oracle's planes are rounded: the suite's tolerance
    if min(W, H) >= 10:
        Bb = oracle.gaussian_blur(B, 1.0)
        c_or, _ = oracle.contrast(Bb, None, oracle.GRADIENT_MAGNITUDE, want_grad=False)
        assert rel_scalar(dio.contrast_ref(B, 1.0, oracle.GRADIENT_MAGNITUDE), c_or) < RTOL


@pytest.mark.parametrize("W,H,sigma", CASES)
@pytest.mark.parametrize("measure", [0, 1, 2])
def test_jt_ref_reproduces_the_oracles_gradient(oracle, W, H, sigma, measure):
    """The oracle's gradient formula on (B, G D) is (2 / N) <Jt - mean term, D>: what the gather kernels compute from Jt."""
    A = poisson_plane(W, H)
    D = np.random.default_rng(W + H).standard_normal((H, W)).astype(np.float32)
    B32, GD32 = oracle.gaussian_blur(A, sigma), oracle.gaussian_blur(D, sigma)
    c_or, g_or = oracle.contrast(B32, GD32[None], measure)
    assert rel_scalar(dio.contrast_ref(A, sigma, measure), c_or) < RTOL
    J = dio.jt_ref(A, sigma, measure)
    D64 = D.astype(np.float64)
    g = 2.0 * np.sum(J * D64) / (W * H)
    scale = 2.0 * np.sum(np.abs(J * D64)) / (W * H)
    if measure == 0:   # (B - mu) against G D - mean(G D): the mean term is mu * sum(G D) / N * 2
        Bd, GD = dio.blurred(A, sigma), dio.blurred(D64, sigma)
        g -= 2.0 * Bd.mean() * GD.mean()
        scale += 2.0 * abs(Bd.mean()) * np.abs(GD).mean()
    assert abs(g - g_or[0]) <= RTOL * scale, (g, g_or[0], scale)


@pytest.mark.parametrize("W,H,sigma", CASES)
@pytest.mark.parametrize("measure", [0, 2])
def test_fp32_passes_against_fp64(oracle, W, H, sigma, measure):
    """e32, the figure the per-pixel bound is made of: the four passes in fp32 stay within the forward error bound of a chain of
    2r + 1-term sums of non-negative terms (four passes, each (2r + 1) products + 2r additions at 2^-24 apiece, first order);
    the Sobel chain has cancelling terms: no a-priori figure is asserted for it
    (test_dropping_one_border_tap_exceeds_the_bound sets the bound against the error it has to resolve)."""
    A = poisson_plane(W, H)
    ref = dio.jt_ref(A, sigma, measure)
    b, e32, scale = dio.bound(A, sigma, measure, ref)
    r = RADII[sigma]
    print("jt %dx%d sigma %g measure %d: e32 %.3e  bound/scale %.3e" % (W, H, sigma, measure, e32, b / scale))
    assert scale == np.abs(ref).max() and b == 8 * max(e32, dio.EPS32) * scale
    assert 0 < e32
    if measure == 0:
        assert e32 <= 4 * (4 * r + 1) * dio.EPS32, e32


def test_compare_set_on_hand_made_planes():
    r = 4
    A = np.zeros((70, 200), np.float32)          # tiles: 4 in x (64, 64, 64, 8), 5 in y (16 x 4, 6)
    assert not dio.compare_set(A, r).any()
    A[0, 0] = 1.0                                 # tile (0, 0): reach 8 -> one tile around it
    m = dio.compare_set(A, r)
    assert m[:32, :128].all() and m.sum() == 32 * 128
    A[:] = 0
    A[69, 199] = -2.0                             # the ragged corner tile (3, 4) and its neighbours
    m = dio.compare_set(A, r)
    assert m[48:, 128:].all() and m.sum() == (70 - 48) * (200 - 128)
    A[:] = 0
    A[40, 100] = 1.0                              # tile (1, 2), radius 12: reach 24 -> one tile in x, two in y
    m = dio.compare_set(A, 12)
    assert m[0:70, 0:192].all() and m.sum() == 70 * 192
    m = dio.compare_set(A, 8)                     # reach 16: one tile each way
    assert m[16:64, 0:192].all() and m.sum() == 48 * 192
    m = dio.compare_set(A, 8, reach=18)           # Sobel: 2r + 2 -> two tile rows
    assert m[0:70, 0:192].all() and m.sum() == 70 * 192
    m = dio.compare_set(A, 0)                     # sigma 0: the tile itself
    assert m[32:48, 64:128].all() and m.sum() == 16 * 64
    # outside the set the reference is exactly zero
    for sigma, measure in ((1.0, 0), (3.0, 0), (2.0, 2)):
        J = dio.jt_ref(A, sigma, measure)
        m = dio.compare_set(A, dio.radius(sigma), dio.jt_reach(sigma, measure))
        assert np.abs(J).max() > 0 and not J[~m].any()


def test_exact_packet_counts(oracle):
    """the raw image of an exact_packet at omega = 0 is the count per pixel (the oracle's fp32 votes)"""
    for W, H in ((10, 10), (65, 17), (100, 70)):
        p = dio.exact_packet(W, H)
        ref = oracle.Frontend(p.W, p.H, p.lut, p.fx, p.fy, p.cx, p.cy, p.batch, 0.0, oracle.VARIANCE)
        ref.set_packet(p.x, p.y, p.t_ns, p.t_ref_ns)
        A = dio.exact_counts(p)
        assert np.array_equal(ref.iwe(np.zeros(3), blur=False), A)
        assert 0.25 * len(p.x) < A.sum() <= len(p.x) and A[1].any() and A[:, 1].any() and A[-3].any() and A[:, -3].any()
        assert len(np.unique(A)) > 5


def test_dropping_one_border_tap_exceeds_the_bound(oracle):
    """the smallest structural error against the bound: the outermost tap of G^T's x pass dropped at ONE pixel (3.5e-5 to
    6.1e-5 of max |Jt| at these radii; the bound is 1.1e-6 to 2.2e-6)"""
    for W, H, sigma in ((65, 17, 1.0), (130, 34, 3.0), (16, 16, 1.7)):
        A = poisson_plane(W, H)
        ref = dio.jt_ref(A, sigma, 0)
        b, e32, scale = dio.bound(A, sigma, 0, ref)
        taps = oracle.gauss_kernel(sigma).astype(np.float64)
        B2 = dio.blur_matrix(H, taps).T @ dio.blurred(A, sigma)          # G^T along y done; the x pass of G^T, one pixel wrong:
        Gx = dio.blur_matrix(W, taps)
        r = dio.radius(sigma)
        y, x = H // 2, W // 2
        bad = ref[y, x] - Gx[x - r, x] * B2[y, x - r]                    # Jt[y, x] = sum_i B2[y, i] Gx[i, x]
        print("drop one tap %dx%d sigma %g: error %.3e of max |Jt|, bound %.3e" % (W, H, sigma, abs(bad - ref[y, x]) / scale, b / scale))
        assert abs(bad - ref[y, x]) > 10 * b, (abs(bad - ref[y, x]) / scale, b / scale)
