"""The adjoint identity behind the Sobel gradient-magnitude contrast's production path, on the CPU.

With I the raw IWE, D_k the raw derivative planes, G the REFLECT_101 Gaussian blur and Sx, Sy cv::Sobel 3x3
(REFLECT_101, Sx = smooth_y o diff_x, Sy = diff_y o smooth_x):

    B = G I,  gx = Sx B,  gy = Sy B
    contrast = (1/N) sum (gx^2 + gy^2)
    grad_k   = (2/N) <D_k, Jt>,   Jt = G^T (Sx^T gx + Sy^T gy)

Every operator is a dense per-axis matrix in fp64 here, borders included, so the transposes are exact.  The reference
side is the oracle's eval(measure=2) (fp32 images, derivative planes).  What image_adjoint_sobel_kernel adds on top of this
identity is the fp32 rounding of Jt.  Not a GPU test: it pins the formula, not the kernel.  Measured on these packets: contrast
within 5.5e-8, gradient within 5.9e-7 relative (the oracle's own fp32 rounding); the bound is the project's RTOL."""
import numpy as np
import pytest

from cmax_slam_amd import synth
from util import RTOL, rel_scalar, rel_vec

OMEGAS = [(0.0, 0.0, 0.0), (0.6, -0.9, 0.4), (-2.0, 1.5, 3.0)]
# (W, H, events, sigmas)
SHAPES = [(240, 180, 30_017, (1.0,)), (70, 40, 3_001, (1.0, 0.0, 2.0)), (64, 16, 700, (1.0,)), (23, 19, 257, (1.0,)),
          (130, 33, 5_000, (1.0,))]


def _reflect101(p, n):
    if n == 1:
        return 0
    while p < 0 or p >= n:
        p = -p if p < 0 else 2 * (n - 1) - p
    return p


def _axis_operator(n, taps):
    """Dense n x n matrix of a 1-D correlation with REFLECT_101 borders: (K v)[p] = sum_j taps[r + j] v[reflect(p + j)]."""
    r = len(taps) // 2
    K = np.zeros((n, n))
    for p in range(n):
        for j in range(-r, r + 1):
            K[p, _reflect101(p + j, n)] += float(taps[r + j])
    return K


def adjoint_gradmag(I, D, taps):
    """(contrast, grad[P], Jt) of the identity above; I: H x W, D: P x H x W."""
    H, W = I.shape
    Gx, Gy = _axis_operator(W, taps), _axis_operator(H, taps)
    Dx, Dy = _axis_operator(W, [-1.0, 0.0, 1.0]), _axis_operator(H, [-1.0, 0.0, 1.0])
    Mx, My = _axis_operator(W, [1.0, 2.0, 1.0]), _axis_operator(H, [1.0, 2.0, 1.0])
    B = Gy @ I @ Gx.T  # rows are y: a y-operator acts from the left, an x-operator from the right (transposed)
    gx = My @ B @ Dx.T
    gy = Dy @ B @ Mx.T
    N = float(W * H)
    contrast = float(np.sum(gx * gx + gy * gy)) / N
    Jt = Gy.T @ (My.T @ gx @ Dx + Dy.T @ gy @ Mx) @ Gx
    grad = np.array([2.0 * float(np.sum(Dk * Jt)) / N for Dk in D])
    return contrast, grad, Jt


def _packet(W, H, n):
    return synth.frontend_packet(n, W, H, 0.83 * W, 0.83 * W, (W - 1) / 2.0, (H - 1) / 2.0, seed=7 + W)


@pytest.mark.parametrize("W,H,n,sigmas", SHAPES)
def test_adjoint_identity_matches_the_oracle(oracle, W, H, n, sigmas):
    p = _packet(W, H, n)
    for sigma in sigmas:
        ref = oracle.Frontend(W, H, p.lut, p.fx, p.fy, p.cx, p.cy, 100, sigma, 2)
        ref.set_packet(p.x, p.y, p.t_ns, p.t_ref_ns)
        taps = oracle.gauss_kernel(sigma).astype(np.float64) if sigma > 0 else np.ones(1)
        for om in OMEGAS:
            c_ref, g_ref = ref.eval(om)
            I, d = ref.iwe(om, deriv=True, blur=False)
            D = np.moveaxis(np.asarray(d, np.float64), -1, 0)
            c, g, _ = adjoint_gradmag(np.asarray(I, np.float64), D, taps)
            ec, eg = rel_scalar(c, c_ref), rel_vec(g, g_ref)
            print(f"{W}x{H} sigma {sigma} omega {om}: contrast {ec:.2e} gradient {eg:.2e}")
            assert ec < RTOL
            assert eg < RTOL
