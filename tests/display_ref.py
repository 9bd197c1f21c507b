"""Test helper: the display path of the reference restated in numpy, and the rule by which an 8-bit image is compared.

What is restated (OpenCV's documented arithmetic, nothing of the reference's text):
  AngVelEstimator::publishEventImage     src/frontend/ang_vel_estimator.cpp:203-233
      hconcat(A, B); normalize(0, 255, NORM_MINMAX, CV_32FC1); 255.f - x; convertTo(CV_8UC1)
  PoseGraphOptimizer::publishEventImage  src/backend/pose_graph_optimizer.cpp:378-413
      normalize(0, 1, NORM_MINMAX, CV_32FC1); pow(gamma); normalize(0, 255, NORM_MINMAX, CV_8UC1); 255 - x; GRAY2BGR
  EventWarper::drawSensorFOV             src/backend/event_pano_warper.cpp:56-79 (warpEventToMap :40-54)
cv::normalize(NORM_MINMAX): scale = (hi - lo > DBL_EPSILON) ? (dmax - dmin) / (hi - lo) : 0, shift = dmin - lo * scale in
fp64; convertTo multiplies and adds in fp32 and, for an 8-bit destination, rounds half to even and saturates.  cv::pow takes
|x| for a non-integer exponent and copies for exponent 1.

Two forms of each chain:
  *_levels      fp64, no intermediate rounding: the real-valued grey level t of every pixel before the final rounding
  *_u8_fp32     the fp32 step-by-step chain (what a host runs today on the fetched fp32 planes)

assert_levels(out, t): a pixel is DECIDED when t lies further than delta = 1e-3 grey levels from the nearest half-integer;
there `out` must equal round(t) exactly.  An undecided pixel may differ by one level.  At most 1 % of the pixels of an image
may be undecided -- a condition on the test's input, asserted here, so that the rule cannot hide a broken kernel.
delta is derived, not tuned: the fp32 chain has at most six roundings of relative size 2^-24 on values <= 255 (<= 1e-4
levels), the device pow is within 16 ulp of a value <= 1 (255 * 16 * 2^-24 = 2.4e-4 levels), taking the extremes of p from
the extremes of v moves the range by <= 1e-6; together < 5e-4 < delta.
The derivation assumes that the pixel at the minimum maps to v = 0 exactly, which holds whenever lo = 0 (every vote image
has an empty pixel) or lo * scale is exact in fp32.  For a plane with lo != 0 the fp32 chain leaves v(lo) = O(2^-24 lo/(hi-lo)),
and pow with gamma < 1 magnifies that (gamma = 0.5: sqrt(6e-8) = 2.4e-4 of the range, 0.06 levels) -- in OpenCV as much as
here.  Test planes with lo != 0 therefore use values for which lo * scale is exact (small dyadic numbers).
"""
import numpy as np

DELTA = 1e-3
MAX_UNDECIDED = 0.01
_EPS = float(np.finfo(np.float64).eps)  # DBL_EPSILON


# ----------------------------------------------------------------------------------------------- fp64 levels
def _unit_range(P):
    """(P - lo) / (hi - lo) in fp64, or None for a plane without a range (cv::normalize's scale = 0)."""
    P = np.asarray(P, np.float64)
    lo, hi = P.min(), P.max()
    if not (hi - lo > _EPS):
        return None
    return (P - lo) / (hi - lo)


def local_pair_levels(A, B):
    """t = 255 - 255 (S - lo) / (hi - lo), S = [A | B]: (H, 2W) fp64.  No range: 255 everywhere."""
    S = np.hstack([np.asarray(A, np.float64), np.asarray(B, np.float64)])
    u = _unit_range(S)
    return np.full(S.shape, 255.0) if u is None else 255.0 - 255.0 * u


def pano_levels(IG, gamma):
    """t = 255 |(IG - lo) / (hi - lo)|^gamma: (Hp, Wp) fp64, BEFORE the inversion (the image is 255 - round(t)).
    No range: 0 everywhere (the image is 255 everywhere)."""
    u = _unit_range(IG)
    return np.zeros(np.shape(IG)) if u is None else 255.0 * np.abs(u) ** float(gamma)


def expected_u8(t, inverted=False):
    r = np.clip(np.rint(t), 0, 255).astype(np.int64)
    return 255 - r if inverted else r


def tie_distance(t):
    """distance of every level from the nearest half-integer (where round() changes its mind)"""
    t = np.asarray(t, np.float64)
    return np.abs(t - (np.floor(t) + 0.5))


def assert_levels(out, t, inverted=False, delta=DELTA, verbose=None):
    """The comparison rule of the module docstring.  Returns (undecided share, pixels that differ from round(t))."""
    out = np.asarray(out)
    assert out.dtype == np.uint8 and out.shape == t.shape, (out.dtype, out.shape, t.shape)
    exp = expected_u8(t, inverted)
    undecided = tie_distance(t) <= delta
    share = float(undecided.mean())
    diff = np.abs(out.astype(np.int64) - exp)
    if verbose:
        print("%s: undecided %.4f %%, differing pixels %d (decided: %d), max |diff| %d" %
              (verbose, 100 * share, int((diff > 0).sum()), int((diff[~undecided] > 0).sum()), int(diff.max())))
    assert share <= MAX_UNDECIDED, "test input has %.2f %% undecided pixels (cap 1 %%): change the input" % (100 * share)
    bad = (diff > 0) & ~undecided
    assert not bad.any(), "%d decided pixels differ, first at %s: got %d, level %.6f" % (
        int(bad.sum()), tuple(np.argwhere(bad)[0]), int(out[tuple(np.argwhere(bad)[0])]), float(t[tuple(np.argwhere(bad)[0])]))
    assert diff.max() <= 1, "an undecided pixel differs by %d levels" % int(diff.max())
    return share, int((diff > 0).sum())


def assert_within_one(out, t, inverted=False):
    """|out - round(t)| <= 1 on every pixel: for planes that are not reproducible from fetch to fetch."""
    out = np.asarray(out)
    assert out.dtype == np.uint8 and out.shape == t.shape
    diff = np.abs(out.astype(np.int64) - expected_u8(t, inverted))
    assert diff.max() <= 1, "max difference %d levels" % int(diff.max())


# ----------------------------------------------------------------------------------------------- fp32 chains
def _norm_ab(lo, hi, dmax):
    d = float(hi) - float(lo)
    scale = dmax / d if d > _EPS else 0.0
    return np.float32(scale), np.float32(-float(lo) * scale)


def _sat_u8(x):
    return np.clip(np.rint(x), 0, 255).astype(np.uint8)


def local_pair_u8_fp32(A, B):
    S = np.hstack([np.asarray(A, np.float32), np.asarray(B, np.float32)])
    a, b = _norm_ab(S.min(), S.max(), 255.0)
    n = S * a + b
    return _sat_u8(np.float32(255.0) - n)


def pano_u8_fp32(IG, gamma):
    IG = np.asarray(IG, np.float32)
    a, b = _norm_ab(IG.min(), IG.max(), 1.0)
    v = IG * a + b
    p = v if float(gamma) == 1.0 else np.abs(v) ** np.float32(gamma)
    a2, b2 = _norm_ab(p.min(), p.max(), 255.0)
    return (255 - _sat_u8(p * a2 + b2).astype(np.int64)).astype(np.uint8)


def gray_to_bgr(img):
    return np.repeat(np.asarray(img)[..., None], 3, axis=2)


# ----------------------------------------------------------------------------------------------- sensor outline
def quat_to_R(q):
    x, y, z, w = np.asarray(q, np.float64) / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def fov_projection(W, H, lut, quat, Wp, Hp):
    """Real-valued panorama coordinates (n, 2) of the sensor's border pixels under the pose `quat` (xyzw): bearing from the
    LUT, rotated, equirectangular projection with fx = Wp / 2 pi, fy = Hp / pi, centre (Wp / 2, Hp / 2)."""
    lut = np.asarray(lut, np.float64).reshape(H, W, 3)
    xs, ys = np.arange(W), np.arange(H)
    border = np.concatenate([lut[0, xs], lut[H - 1, xs], lut[ys, 0], lut[ys, W - 1]])
    r = border @ quat_to_R(quat).T
    phi = np.arctan2(r[:, 0], r[:, 2])
    theta = np.arcsin(r[:, 1] / np.linalg.norm(r, axis=1))
    fx = (Wp / 360.0) * 180.0 / np.pi
    fy = (Hp / 180.0) * 180.0 / np.pi
    return np.stack([Wp / 2.0 + phi * fx, Hp / 2.0 + theta * fy], axis=1)


def fov_pixels(W, H, lut, quat, Wp, Hp):
    """(set of (x, y) panorama pixels of the outline, smallest distance of any projected coordinate from a rounding tie).
    cv::Point2d -> cv::Point rounds half to even; points outside the panorama are skipped."""
    p = fov_projection(W, H, lut, quat, Wp, Hp)
    tie = float(tie_distance(p).min())
    r = np.rint(p).astype(np.int64)
    ok = (r[:, 0] >= 0) & (r[:, 0] < Wp) & (r[:, 1] >= 0) & (r[:, 1] < Hp)
    return set(map(tuple, r[ok])), tie


# ----------------------------------------------------------------------------------------------- inputs
def vote_image(Wp, Hp, n_votes, seed):
    """A seeded bilinear vote image (fp32 accumulation like the splat's): arcs of votes across the band, a share of the
    pixels non-zero, many votes per touched pixel."""
    rng = np.random.default_rng(seed)
    n_arcs = 40
    per = n_votes // n_arcs
    img = np.zeros(Hp * Wp, np.float64)
    for _ in range(n_arcs):
        x0, y0 = rng.uniform(0, Wp), rng.uniform(0.2 * Hp, 0.8 * Hp)
        ang, length = rng.uniform(0, 2 * np.pi), rng.uniform(0.1, 0.5) * Wp
        s = rng.uniform(0, 1, per)
        x = (x0 + s * length * np.cos(ang) + rng.normal(0, 2.0, per)) % (Wp - 1)
        y = np.clip(y0 + s * length * np.sin(ang) * 0.3 + rng.normal(0, 2.0, per), 0, Hp - 1.001)
        ix, iy = np.floor(x).astype(np.int64), np.floor(y).astype(np.int64)
        dx, dy = x - ix, y - iy
        for ox, oy, wgt in ((0, 0, (1 - dx) * (1 - dy)), (1, 0, dx * (1 - dy)), (0, 1, (1 - dx) * dy), (1, 1, dx * dy)):
            np.add.at(img, (iy + oy) * Wp + ix + ox, wgt.astype(np.float32))
    return img.reshape(Hp, Wp).astype(np.float32)
