"""Test helper: the image operators of the adjoint pass as explicit matrices in fp64 (numpy and oracle.pyoracle only).

The forward image is B = Gy A Gx^T, with G the REFLECT_101 Gaussian of cv::GaussianBlur(Size(0, 0), sigma) per axis.  The plane every
gradient gather reads is Jt = Gy^T (Gy A Gx^T) Gx; for the gradient-magnitude contrast the Sobel normal operator
Sx^T Sx + Sy^T Sy sits between G and G^T (Sx = smooth_y o diff_x, Sy = diff_y o smooth_x, cv::Sobel 3 x 3, REFLECT_101).

A REFLECT_101 filter of radius b is a band matrix of half-width b (a tap mirrored at the border lands inside the band), so every
operator here is held as a Banded: dense() gives the L x L array, dot() applies it without forming one (sides above 512).

jt_ref applies the operators in fp64; jt_fp32 applies the same four (eight) passes with every product and every partial sum
rounded to fp32: the reference side's own rounding error, from which tests take their per-pixel bound (bound()).
"""
import numpy as np

from oracle import pyoracle as po

TILE_X, TILE_Y = 64, 16  # tile of the image passes: the granularity at which a pass may skip work
DENSE_MAX = 512          # blur_matrix returns an ndarray up to this side, a Banded above


def reflect101(p, L):
    """BORDER_REFLECT_101 (gfedcb|abcdefgh|gfedcba) of the integer array p on [0, L)"""
    p = np.asarray(p).copy()
    if L == 1:
        return np.zeros_like(p)
    while True:
        lo, hi = p < 0, p >= L
        if not (lo.any() or hi.any()):
            return p
        p[lo] = -p[lo]
        p[hi] = 2 * (L - 1) - p[hi]


class Banded:
    """L x L matrix with M[i, j] = band[i, j - i + b] for |j - i| <= b, zero elsewhere."""

    def __init__(self, band):
        self.band = np.asarray(band)
        self.L, w = self.band.shape
        self.b = (w - 1) // 2

    @classmethod
    def from_filter(cls, L, taps, dtype=np.float64):
        """out[i] = sum_k taps[k] in[reflect101(i - r + k)]; taps mirrored onto one column add up in `dtype`"""
        taps = np.asarray(taps)
        r = (len(taps) - 1) // 2
        if L <= r:
            raise ValueError("side %d does not hold a single reflection of radius %d" % (L, r))
        band = np.zeros((L, 2 * r + 1), dtype)
        i = np.arange(L)
        for k in range(len(taps)):
            j = reflect101(i - r + k, L)
            np.add.at(band, (i, j - i + r), np.asarray(taps[k], dtype))
        return cls(band)

    @property
    def T(self):
        L, b = self.L, self.b
        out = np.zeros_like(self.band)
        for e in range(2 * b + 1):  # M^T[j, j + e - b] = M[j + e - b, j] = band[j + e - b, 2b - e]
            j = np.arange(max(0, b - e), min(L, L + b - e))
            out[j, e] = self.band[j + e - b, 2 * b - e]
        return Banded(out)

    def astype(self, dtype):
        return Banded(self.band.astype(dtype))

    def dense(self):
        M = np.zeros((self.L, self.L), self.band.dtype)
        for d in range(2 * self.b + 1):
            i = np.arange(max(0, self.b - d), min(self.L, self.L + self.b - d))
            M[i, i + d - self.b] = self.band[i, d]
        return M

    def dot(self, X):
        """M @ X for X of shape (L, n); products and the running sum (diagonal by diagonal) stay in X's dtype"""
        X = np.asarray(X)
        L, b = self.L, self.b
        assert X.shape[0] == L, (X.shape, L)
        band = self.band.astype(X.dtype)
        out = np.zeros_like(X)
        for d in range(2 * b + 1):
            lo, hi = max(0, b - d), min(L, L + b - d)
            if hi > lo:
                out[lo:hi] += band[lo:hi, d, None] * X[lo + d - b:hi + d - b]
        return out


def _dot(M, X):
    return M.dot(X) if isinstance(M, Banded) else M @ X


def _T(M):
    return M.T


def apply2(My, Mx, A):
    """My A Mx^T: My along the rows' index (y), Mx along the columns' (x)"""
    return _dot(Mx, _dot(My, A).T).T


def blur_matrix(L, taps, banded=None):
    """The L x L REFLECT_101 operator of a filter with the given fp32 taps, in fp64: an ndarray for L <= 512, a Banded above
    (banded=True / False forces one form)."""
    B = Banded.from_filter(L, np.asarray(taps, np.float32).astype(np.float64))
    if banded is None:
        banded = L > DENSE_MAX
    return B if banded else B.dense()


def sobel_matrices(L, banded=None):
    """(smooth, diff) of cv::Sobel 3 x 3 along one axis with REFLECT_101: [1 2 1] and [-1 0 1]"""
    return blur_matrix(L, [1.0, 2.0, 1.0], banded), blur_matrix(L, [-1.0, 0.0, 1.0], banded)


def radius(sigma):
    return (len(po.gauss_kernel(sigma)) - 1) // 2


def jt_reach(sigma, measure):
    """how far a non-zero pixel of A reaches into Jt, per axis: 2r, or 2r + 2 through the Sobel normal operator"""
    return 2 * radius(sigma) + (2 if measure == po.GRADIENT_MAGNITUDE else 0)


def _operators(H, W, sigma, dtype):
    taps = po.gauss_kernel(sigma)
    big = max(H, W) > DENSE_MAX

    def mk(L, t):
        B = Banded.from_filter(L, np.asarray(t, np.float32).astype(dtype), dtype)
        return B if (big or dtype != np.float64) else B.dense()

    ops = {"Gy": mk(H, taps), "Gx": mk(W, taps)}
    for ax, L in (("y", H), ("x", W)):
        ops["S" + ax], ops["D" + ax] = mk(L, [1.0, 2.0, 1.0]), mk(L, [-1.0, 0.0, 1.0])
    return ops


def _sobel_normal(o, B):
    gx = apply2(o["Sy"], o["Dx"], B)
    gy = apply2(o["Dy"], o["Sx"], B)
    return apply2(_T(o["Sy"]), _T(o["Dx"]), gx) + apply2(_T(o["Dy"]), _T(o["Sx"]), gy)


def _jt(A, sigma, measure, dtype):
    A = np.asarray(A, dtype)
    H, W = A.shape
    o = _operators(H, W, sigma, dtype)
    B = apply2(o["Gy"], o["Gx"], A)
    if measure == po.GRADIENT_MAGNITUDE:
        B = _sobel_normal(o, B)
    return apply2(_T(o["Gy"]), _T(o["Gx"]), B)


def blurred(A, sigma):
    """B = Gy A Gx^T in fp64"""
    A = np.asarray(A, np.float64)
    o = _operators(A.shape[0], A.shape[1], sigma, np.float64)
    return apply2(o["Gy"], o["Gx"], A)


def jt_ref(A, sigma, measure):
    """Gy^T (Gy A Gx^T) Gx in fp64; measure 2: Gy^T N(Gy A Gx^T) Gx with N = Sx^T Sx + Sy^T Sy"""
    return _jt(A, sigma, measure, np.float64)


def jt_fp32(A, sigma, measure):
    """the same passes, one after the other, in fp32 (taps, products, running sums)"""
    return _jt(A, sigma, measure, np.float32)


def contrast_ref(A, sigma, measure):
    """fp64 contrast of B = Gy A Gx^T: population variance, mean square, or mean of gx^2 + gy^2 (cv::Sobel)"""
    A = np.asarray(A, np.float64)
    o = _operators(A.shape[0], A.shape[1], sigma, np.float64)
    B = apply2(o["Gy"], o["Gx"], A)
    if measure == po.GRADIENT_MAGNITUDE:
        gx, gy = apply2(o["Sy"], o["Dx"], B), apply2(o["Dy"], o["Sx"], B)
        return float(np.mean(gx * gx + gy * gy))
    if measure == po.MEAN_SQUARE:
        return float(np.mean(B * B))
    return float(np.mean((B - B.mean()) ** 2))


def compare_set(A, r, reach=None):
    """Boolean (H, W) mask: the pixels of every 64 x 16 tile within ceil(reach / 64) tiles in x and ceil(reach / 16) in y of a tile
    that holds a non-zero pixel of A (reach = 2r by default; 2r + 2 for Sobel).  An image pass may skip every other tile: Jt is
    exactly zero there (no non-zero pixel within reach), and what the device holds is whatever an earlier pass left."""
    A = np.asarray(A)
    H, W = A.shape
    if reach is None:
        reach = 2 * r
    ty, tx = -(-H // TILE_Y), -(-W // TILE_X)
    pad = np.zeros((ty * TILE_Y, tx * TILE_X), bool)
    pad[:H, :W] = A != 0
    flags = pad.reshape(ty, TILE_Y, tx, TILE_X).any(axis=(1, 3))
    ny, nx = -(-reach // TILE_Y), -(-reach // TILE_X)
    act = np.zeros_like(flags)
    for y, x in zip(*np.nonzero(flags)):
        act[max(0, y - ny):y + ny + 1, max(0, x - nx):x + nx + 1] = True
    return np.repeat(np.repeat(act, TILE_Y, axis=0), TILE_X, axis=1)[:H, :W]


EPS32 = 2.0 ** -24


def bound(A, sigma, measure, ref=None):
    """(absolute per-pixel bound, e32, max |jt_ref|): 8 max(e32, 2^-24) max |jt_ref| with e32 = max |jt_fp32 - jt_ref| / max |jt_ref|.
    Nothing in it comes from a device.  The factor 8: a kernel that adds the same 2r + 1 (composite operator: 4r + 1) terms in
    another order, or contracted to FMAs."""
    ref = jt_ref(A, sigma, measure) if ref is None else ref
    scale = float(np.abs(ref).max())
    if scale == 0.0:
        return 0.0, 0.0, 0.0
    e32 = float(np.abs(jt_fp32(A, sigma, measure).astype(np.float64) - ref).max()) / scale
    return 8.0 * max(e32, EPS32) * scale, e32, scale


def worst_pixel(dev, ref, mask):
    """(error, y, x) of the largest |dev - ref| inside mask"""
    err = np.where(mask, np.abs(np.asarray(dev, np.float64) - ref), -1.0)
    y, x = np.unravel_index(int(np.argmax(err)), err.shape)
    return float(err[y, x]), int(y), int(x)


def describe_pixel(y, x, H, W):
    """where a pixel sits: inside its tile and relative to the four image borders (what locates a wrong fold)"""
    return ("pixel (x %d, y %d): tile (%d, %d), position in tile (%d, %d); to the borders: left %d, right %d, top %d, bottom %d"
            % (x, y, x // TILE_X, y // TILE_Y, x % TILE_X, y % TILE_Y, x, W - 1 - x, y, H - 1 - y))


def exact_packet(W, H, seed=None):
    """Integer-pixel events, uneven counts per pixel (blobs of different weight over a sparse uniform floor), fx = fy = 256, integer
    cx, cy, omega = 0: the warp gives u = x exactly, the bilinear weights are 1 / 0 / 0 / 0 and the raw image is a count per pixel
    (exact_counts) whatever the order of the atomics.  seed None: 1000 W + H."""
    from cmax_slam_amd import synth
    rng = np.random.default_rng(1000 * W + H if seed is None else seed)
    n = max(20_000, (W * H * 2) // 3)
    nb = 40
    cxs, cys = rng.uniform(0, W, nb), rng.uniform(0, H, nb)
    spread = rng.uniform(1.5, max(1.5, 0.08 * W), nb)  # (sides below 19: every blob at the least spread)
    which = rng.choice(nb, size=n, p=rng.dirichlet(np.ones(nb)))
    x = np.rint(cxs[which] + spread[which] * rng.standard_normal(n))
    y = np.rint(cys[which] + spread[which] * rng.standard_normal(n))
    floor = rng.random(n) < 0.15
    x[floor] = rng.integers(0, W, int(floor.sum()))
    y[floor] = rng.integers(0, H, int(floor.sum()))
    x = np.clip(x, 0, W - 2).astype(np.uint16)  # (the vote's 2 x 2 cell stays inside the image)
    y = np.clip(y, 0, H - 2).astype(np.uint16)
    T = 0.05
    t_ns = synth.T0_NS + np.sort(np.floor(rng.random(n) * T * 1e9).astype(np.int64))
    return synth.FrontendPacket(W, H, 256.0, 256.0, float(W // 2), float(H // 2), x, y, t_ns, synth.T0_NS + int(round(T / 2 * 1e9)),
                                np.zeros(3))


def exact_counts(p):
    """the raw image of an exact_packet at omega = 0, by counting: (H, W) fp32 (counts stay far below 2^24).  An event votes when
    1 <= x < W - 2 and 1 <= y < H - 2 (the reference's rule, oracle/frontend.c): a frame of one pixel (two on the far sides) stays
    empty, and the folds of the border taps act on the rows and columns next to it."""
    x, y = p.x.astype(np.int64), p.y.astype(np.int64)
    keep = (1 <= x) & (x < p.W - 2) & (1 <= y) & (y < p.H - 2)
    A = np.zeros((p.H, p.W), np.int64)
    np.add.at(A, (y[keep], x[keep]), 1)
    assert A.max() < 2 ** 24
    return A.astype(np.float32)
