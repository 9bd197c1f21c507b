"""CPU: the numpy restatement of the display path (tests/display_ref.py) against cases worked out by hand, and the
surface of the feature -- the two entry points are exported, bound and reachable -- which fails without it."""
import ctypes as C
import inspect

import numpy as np
import pytest

import display_ref as dr


# ----------------------------------------------------------------------------------------------- the helper itself
def test_pair_levels_2x2_by_hand():
    A = np.array([[0.0, 1.0], [2.0, 4.0]])
    B = np.array([[4.0, 3.0], [0.0, 0.5]])
    # lo = 0, hi = 4: t = 255 - 63.75 S
    want = np.array([[255.0, 191.25, 0.0, 63.75], [127.5, 0.0, 255.0, 223.125]])
    t = dr.local_pair_levels(A, B)
    np.testing.assert_allclose(t, want, rtol=0, atol=1e-12)
    out = dr.local_pair_u8_fp32(A, B)
    assert out.dtype == np.uint8 and out.shape == (2, 4)
    # 127.5 is a tie: round half to even -> 128; 191.25 -> 191; 63.75 -> 64; 223.125 -> 223
    np.testing.assert_array_equal(out, [[255, 191, 0, 64], [128, 0, 255, 223]])


def test_pano_levels_3x4_by_hand():
    IG = np.array([[0.0, 1.0, 4.0, 9.0], [16.0, 0.0, 0.0, 4.0], [1.0, 9.0, 16.0, 0.25]])
    # lo = 0, hi = 16, gamma = 0.5: t = 255 sqrt(IG) / 4
    want = 255.0 * np.sqrt(IG) / 4.0
    np.testing.assert_allclose(dr.pano_levels(IG, 0.5), want, rtol=0, atol=1e-12)
    out = dr.pano_u8_fp32(IG, 0.5)
    # levels 0, 63.75, 127.5 (tie -> 128), 191.25, 255, 31.875 -> inverted
    np.testing.assert_array_equal(out, 255 - np.array([[0, 64, 128, 191], [255, 0, 0, 128], [64, 191, 255, 32]]))


def test_constant_planes_are_white():
    for val in (0.0, 3.5, -2.0):
        P = np.full((5, 7), val, np.float32)
        assert (dr.local_pair_levels(P, P) == 255.0).all()
        assert (dr.local_pair_u8_fp32(P, P) == 255).all()
        for g in (0.5, 1.0, 2.2):
            assert (dr.pano_levels(P, g) == 0.0).all()
            assert (dr.pano_u8_fp32(P, g) == 255).all()


def test_negative_values_and_signed_zero():
    IG = np.array([[-2.0, -0.0, 0.0, 2.0], [6.0, -1.0, 3.0, 0.0]], np.float32)
    # lo = -2, hi = 6: u = (IG + 2) / 8
    u = np.array([[0.0, 0.25, 0.25, 0.5], [1.0, 0.125, 0.625, 0.25]])
    np.testing.assert_allclose(dr.pano_levels(IG, 1.0), 255.0 * u, rtol=0, atol=1e-12)
    np.testing.assert_allclose(dr.pano_levels(IG, 2.2), 255.0 * u ** 2.2, rtol=0, atol=1e-10)
    out = dr.pano_u8_fp32(IG, 1.0)
    assert out[0, 1] == out[0, 2] == out[1, 3]  # -0 and +0 are one value
    np.testing.assert_array_equal(out, 255 - np.array([[0, 64, 64, 128], [255, 32, 159, 64]]))  # 63.75, 127.5, 31.875, 159.375


def test_gamma_one_is_the_linear_map():
    IG = dr.vote_image(96, 48, 3000, seed=5)
    lo, hi = float(IG.min()), float(IG.max())
    np.testing.assert_allclose(dr.pano_levels(IG, 1.0), 255.0 * (IG.astype(np.float64) - lo) / (hi - lo), rtol=0, atol=1e-10)


@pytest.mark.parametrize("gamma", [0.5, 0.75, 1.0])
def test_fp32_chain_passes_the_rule_on_a_vote_map(gamma):
    """The fp32 numpy chain against the fp64 levels on a 1024 x 512 map of 400 000 bilinear votes: every decided pixel exact,
    far fewer than 1 % undecided."""
    IG = dr.vote_image(1024, 512, 400_000, seed=11)
    assert 0.05 < (IG != 0).mean() < 0.6
    share, ndiff = dr.assert_levels(dr.pano_u8_fp32(IG, gamma), dr.pano_levels(IG, gamma), inverted=True,
                                    verbose="gamma %.2f" % gamma)
    assert share < 0.002 and ndiff <= 16


def test_fp32_pair_chain_passes_the_rule():
    A = dr.vote_image(240, 180, 30_000, seed=3)
    B = dr.vote_image(240, 180, 30_000, seed=4)
    dr.assert_levels(dr.local_pair_u8_fp32(A, B), dr.local_pair_levels(A, B))


def test_rule_rejects_a_wrong_image():
    IG = dr.vote_image(256, 128, 30_000, seed=7)
    t = dr.pano_levels(IG, 0.75)
    good = dr.pano_u8_fp32(IG, 0.75)
    dr.assert_levels(good, t, inverted=True)
    bad = good.copy()
    y, x = np.argwhere(dr.tie_distance(t) > 0.4)[0]
    bad[y, x] ^= 1
    with pytest.raises(AssertionError):
        dr.assert_levels(bad, t, inverted=True)       # one decided pixel off by one level
    with pytest.raises(AssertionError):
        dr.assert_levels(good, t, inverted=False)     # the inversion forgotten
    with pytest.raises(AssertionError):               # an input made of ties is refused, whatever the image
        dr.assert_levels(np.full((4, 4), 128, np.uint8), np.full((4, 4), 127.5), inverted=False)


def test_fov_pixels_identity_pose_corners_by_hand():
    """8 x 6 pinhole sensor, f = 4, centre (3.5, 2.5), identity pose, 64 x 32 panorama: fx = 64 / 2 pi, fy = 32 / pi.
    A corner (x, y) has the bearing ((x - 3.5) / 4, (y - 2.5) / 4, 1):
      phi = atan(+-0.875) = +-0.7188300,  theta = asin(+-0.625 / sqrt(0.875^2 + 0.625^2 + 1)) = +-0.4396510
      px = 32 + phi * 10.1859164 = 32 +- 7.3219    py = 16 + theta * 10.1859164 = 16 +- 4.4783
    -> (25, 12), (39, 12), (25, 20), (39, 20)."""
    from cmax_slam_amd import synth
    W, H, Wp, Hp = 8, 6, 64, 32
    lut = synth.pinhole_lut(W, H, 4.0, 4.0, 3.5, 2.5)
    pix, tie = dr.fov_pixels(W, H, lut, (0, 0, 0, 1), Wp, Hp)
    assert {(25, 12), (39, 12), (25, 20), (39, 20)} <= pix
    assert tie > 1e-9
    p = dr.fov_projection(W, H, lut, (0, 0, 0, 1), Wp, Hp)
    np.testing.assert_allclose(p[0], [32 - 7.3219, 16 - 4.4783], atol=1e-4)           # (0, 0)
    np.testing.assert_allclose(p[2 * W - 1], [32 + 7.3219, 16 + 4.4783], atol=1e-4)   # (W-1, H-1)
    assert len(p) == 2 * (W + H)
    # the outline is the closed border, symmetric about the panorama's centre; its horizontal edges bow away from the equator:
    # mid-edge (x = 3 or 4) the bearing is (+-0.125, +-0.625, 1), theta = asin(0.625 / 1.18585) = 0.55513 -> 16 +- 5.65
    xs, ys = np.array(sorted(pix)).T
    assert xs.min() == 25 and xs.max() == 39 and ys.min() == 10 and ys.max() == 22
    assert {(Wp - x, Hp - y) for x, y in pix} == pix
    # a yaw of pi moves the outline across the +-pi seam; nothing falls outside, nothing is lost
    pix_s, _ = dr.fov_pixels(W, H, lut, (0, np.sin(np.pi / 2 - 0.01), 0, np.cos(np.pi / 2 - 0.01)), Wp, Hp)
    xs = np.array(sorted(pix_s))[:, 0]
    assert xs.min() <= 7 and xs.max() >= 57 and not ((xs > 10) & (xs < 54)).any()


# ----------------------------------------------------------------------------------------------- the feature's surface
@pytest.fixture(scope="module")
def L():
    from cmax_slam_amd import _lib
    _lib.build()
    return _lib.lib()


def test_entry_points_are_exported_and_bound(L):
    from cmax_slam_amd import _lib, evaluator
    raw = C.CDLL(_lib.SO_PATH)
    u8p = C.POINTER(C.c_uint8)
    for name, args in (("cmx_frontend_render_display", [_lib.ctx_p, _lib.c_dp, u8p]),
                       ("cmx_backend_render_map", [_lib.ctx_p, C.c_double, _lib.c_dp, u8p])):
        assert hasattr(raw, name), "libcmaxhip.so does not export %s" % name
        assert name in _lib.SYMBOLS, "%s missing from the binding table" % name
        assert _lib.SYMBOLS[name] == (C.c_int, args)
    fe = inspect.signature(evaluator.FrontendEvaluator.publishEventImage)
    be = inspect.signature(evaluator.BackendEvaluator.publishEventImage)
    assert list(fe.parameters) == ["self", "ang_vel"]
    assert list(be.parameters) == ["self", "gamma", "fov_quat"]
    assert be.parameters["gamma"].default == 0.75 and be.parameters["fov_quat"].default is None


def test_null_context_is_a_state_error(L):
    from cmax_slam_amd import _lib
    out = np.zeros(16, np.uint8)
    om = (C.c_double * 3)(0.0, 0.0, 0.0)
    q = (C.c_double * 4)(0.0, 0.0, 0.0, 1.0)
    o = out.ctypes.data_as(C.POINTER(C.c_uint8))
    assert L.cmx_frontend_render_display(None, om, o) == _lib.ERR_STATE
    assert L.cmx_backend_render_map(None, 0.75, None, o) == _lib.ERR_STATE
    assert L.cmx_backend_render_map(None, 0.75, q, o) == _lib.ERR_STATE
    assert (out == 0).all()
