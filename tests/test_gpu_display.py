"""-m gpu: the display path on the device -- cmx_frontend_render_display (AngVelEstimator::publishEventImage,
src/frontend/ang_vel_estimator.cpp:203-233) and cmx_backend_render_map (PoseGraphOptimizer::publishEventImage,
src/backend/pose_graph_optimizer.cpp:378-413, with EventWarper::drawSensorFOV, src/backend/event_pano_warper.cpp:56-79)
against the fp64 levels of tests/display_ref.py under its comparison rule (decided pixels exact, undecided within one level,
at most 1 % undecided), and the promise that a render changes no later result."""
import ctypes as C

import numpy as np
import pytest

import display_ref as dr
from cmax_slam_amd import _lib, synth
from util import RTOL, rel_scalar, rel_vec

pytestmark = pytest.mark.gpu

U8P = C.POINTER(C.c_uint8)


def _qx(a):
    return (np.sin(a / 2), 0.0, 0.0, np.cos(a / 2))


def _qy(a):
    return (0.0, np.sin(a / 2), 0.0, np.cos(a / 2))


def _packet(kind):
    if kind == "240x180":
        return synth.frontend_packet(30_011, 240, 180, 200.0, 200.0, 119.5, 89.5, seed=71)
    return synth.config2()  # 640 x 480, 1 000 000 events


def _set_packet(fe, p):
    fe.set_packet(p.x, p.y, p.t_ns, p.t_ref_ns, p.fx, p.fy, p.cx, p.cy, p.batch, p.sigma, 0)


# ------------------------------------------------------------------------------------------------ front end
@pytest.mark.parametrize("kind", ["240x180", "640x480"])
def test_frontend_pair_deterministic_planes(hip, kind):
    """With CMX_OPT_DETERMINISTIC the blur-free planes are reproducible bit for bit (asserted first), so the planes fetched
    from the context are the planes the render saw: the full rule applies."""
    p = _packet(kind)
    fe = hip.FrontendEvaluator(p.W, p.H, p.lut)
    fe.set_deterministic()
    _set_packet(fe, p)
    for om in (np.zeros(3), np.asarray(p.omega_true, np.float64)):
        A = fe.computeImageOfWarpedEvents(np.zeros(3), blur=False)
        B = fe.computeImageOfWarpedEvents(om, blur=False)
        np.testing.assert_array_equal(A, fe.computeImageOfWarpedEvents(np.zeros(3), blur=False))
        np.testing.assert_array_equal(B, fe.computeImageOfWarpedEvents(om, blur=False))
        out = fe.publishEventImage(om)
        assert out.shape == (p.H, 2 * p.W) and out.dtype == np.uint8
        dr.assert_levels(out, dr.local_pair_levels(A, B), verbose="front end %s omega %s" % (kind, om))
        assert out.min() == 0 and out.max() == 255
        if not om.any():
            np.testing.assert_array_equal(out[:, :p.W], out[:, p.W:])
        np.testing.assert_array_equal(out, fe.publishEventImage(om))  # and the render itself is reproducible


@pytest.mark.parametrize("path", ["production", "reference-shaped"])
def test_frontend_pair_atomic_planes(hip, path):
    """Without the option the planes are sums of fp32 atomics in arrival order and differ from fetch to fetch in the last
    bits: every pixel within one level of the levels of a separately fetched pair."""
    p = _packet("240x180")
    cls = hip.FrontendEvaluator if path == "production" else hip.reference_shaped.FrontendEvaluator
    fe = cls(p.W, p.H, p.lut)
    _set_packet(fe, p)
    for om in (np.zeros(3), np.asarray(p.omega_true, np.float64)):
        out = fe.publishEventImage(om)
        A = fe.computeImageOfWarpedEvents(np.zeros(3), blur=False)
        B = fe.computeImageOfWarpedEvents(om, blur=False)
        dr.assert_within_one(out, dr.local_pair_levels(A, B))
        assert out.min() == 0 and out.max() == 255


def test_frontend_empty_half_empty_pair_and_ragged_width(hip):
    """A packet whose events all sit on one interior pixel and, at the rendered omega, all warp out of the image (a quarter
    turn between the events and the reference time): the compensated half is empty and white, the raw half holds one black
    pixel.  The same packet on the last pixel of the sensor casts no vote at all (the bilinear vote needs a neighbour):
    255 everywhere.  Widths 64 (packed stores) and 66 (not a multiple of 4: the byte path)."""
    H = 48
    for W in (64, 66):
        f, cx, cy = 80.0, (W - 1) / 2, (H - 1) / 2
        fe = hip.FrontendEvaluator(W, H, synth.pinhole_lut(W, H, f, f, cx, cy))
        fe.set_deterministic()
        n = 500
        t = np.arange(n, dtype=np.int64) * 1000 + 2_000_000_000
        om = np.array([0.0, np.pi / 2, 0.0])
        for (ex, ey), votes in (((W - 5, H - 7), 1), ((W - 1, H - 1), 0)):
            x, y = np.full(n, ex, np.uint16), np.full(n, ey, np.uint16)
            fe.set_packet(x, y, t, int(t[0]) - 1_000_000_000, f, f, cx, cy, 100, 0.0, 0)
            A = fe.computeImageOfWarpedEvents(np.zeros(3), blur=False)
            B = fe.computeImageOfWarpedEvents(om, blur=False)
            assert B.max() == 0 and (A > 0).sum() == votes, "the test's packet is not what it was built to be"
            out = fe.publishEventImage(om)
            dr.assert_levels(out, dr.local_pair_levels(A, B))
            assert (out[:, W:] == 255).all() and (out == 255).sum() == out.size - votes
            if votes:
                assert out[ey, ex] == 0


# ------------------------------------------------------------------------------------------------ panorama, mono
GAMMAS = (0.5, 0.75, 1.0, 2.2)


@pytest.mark.parametrize("Wp,Hp", [(512, 256), (1024, 512)])
def test_panorama_of_a_built_map(hip, Wp, Hp):
    """A map built as the back end builds it (a window, one evaluation, updateIG), then rendered at four gammas."""
    w = synth.backend_window(40_003, 240, 180, 200.0, 200.0, 119.5, 89.5, Wp, Hp, 2, 5, 1, 0.2, seed=21)
    be = hip.BackendEvaluator(w.W, w.H, w.lut, w.Wp, w.Hp)
    be.set_window(w.x, w.y, w.t_ns, 2, w.knots_init, w.start_ns, w.dt_ns, w.num_fixed, w.t_next_win_beg_ns)
    be.eval(np.full(w.P, 0.002), False)
    be.updateIG(1)
    IG = be.getIG()
    assert IG.max() > 0 and (IG == 0).any()
    for g in GAMMAS:
        out = be.publishEventImage(g)
        assert out.shape == (Hp, Wp) and out.dtype == np.uint8
        dr.assert_levels(out, dr.pano_levels(IG, g), inverted=True, verbose="%dx%d gamma %.2f" % (Wp, Hp, g))
        assert out.min() == 0 and out.max() == 255
    np.testing.assert_array_equal(be.getIG(), IG)


def test_panorama_4096x2048_loaded_map(hip):
    w = synth.backend_window(2_000, 240, 180, 200.0, 200.0, 119.5, 89.5, 4096, 2048, 2, 5, 1, 0.2, seed=3)
    be = hip.BackendEvaluator(w.W, w.H, w.lut, 4096, 2048)
    IG = dr.vote_image(4096, 2048, 3_000_000, seed=13)
    be.setIG(IG)
    for g in GAMMAS:
        dr.assert_levels(be.publishEventImage(g), dr.pano_levels(IG, g), inverted=True, verbose="4096x2048 gamma %.2f" % g)


def _dyadic_plane(Wp, Hp, seed):
    """Integers in [-8, 56], some zeros of either sign: lo = -8, hi = 56, scale = 1 / 64, so lo * scale and every
    v = IG * a + b are exact in fp32 (see display_ref's docstring).  24 and 8 are left out: u = (k + 8) / 64 makes
    255 u = 127.5 at k = 24 and 255 sqrt(u) = 127.5 at k = 8, ties at gamma 1 and 0.5."""
    rng = np.random.default_rng(seed)
    vals = np.array([k for k in range(-8, 57) if k not in (8, 24)], np.float32)
    P = rng.choice(vals, size=(Hp, Wp)).astype(np.float32)
    P[0, 0], P[Hp - 1, Wp - 1] = -8.0, 56.0
    P[rng.integers(0, Hp, 50), rng.integers(1, Wp - 1, 50)] = -0.0
    P[rng.integers(0, Hp, 50), rng.integers(1, Wp - 1, 50)] = 0.0
    return P


@pytest.mark.parametrize("Wp,Hp", [(512, 256), (500, 250), (501, 251)])
def test_panorama_edge_planes(hip, Wp, Hp):
    """All-zero (also straight after create), constant, negative values with -0.0, a single pixel, and shapes whose width is
    not a multiple of 64 (500) or whose pixel count is not a multiple of 4 (501 x 251: the loads and packed stores meet
    their tails), mono and BGR."""
    lut = synth.pinhole_lut(240, 180, 200.0, 200.0, 119.5, 89.5)
    be = hip.BackendEvaluator(240, 180, lut, Wp, Hp)
    q = _qx(np.pi / 3)
    white = np.full((Hp, Wp), 255, np.uint8)
    np.testing.assert_array_equal(be.publishEventImage(0.75), white)          # straight after create: no window at all
    be.setIG(np.zeros((Hp, Wp), np.float32))
    np.testing.assert_array_equal(be.publishEventImage(0.5), white)
    be.setIG(np.full((Hp, Wp), 3.5, np.float32))
    for g in (0.75, 1.0):
        np.testing.assert_array_equal(be.publishEventImage(g), white)
    bgr = be.publishEventImage(0.75, q)
    pix, _ = dr.fov_pixels(240, 180, lut, q, Wp, Hp)
    on = np.zeros((Hp, Wp), bool)
    on[[y for _, y in pix], [x for x, _ in pix]] = True
    assert (bgr[~on] == 255).all() and (bgr[on] == (255, 0, 0)).all()

    P = _dyadic_plane(Wp, Hp, seed=Wp)
    be.setIG(P)
    for g in (0.5, 1.0, 2.2):
        out = be.publishEventImage(g)
        dr.assert_levels(out, dr.pano_levels(P, g), inverted=True, verbose="dyadic %dx%d gamma %.1f" % (Wp, Hp, g))
        assert len(set(out[P == 0].tolist())) == 1                            # -0 and +0 are one value
        assert out[0, 0] == 255 and out[Hp - 1, Wp - 1] == 0

    one = np.zeros((Hp, Wp), np.float32)
    one[Hp - 1, Wp - 1] = 7.25                                                # the very last pixel: in the tail when there is one
    be.setIG(one)
    out = be.publishEventImage(0.75)
    assert out[Hp - 1, Wp - 1] == 0 and (out == 255).sum() == out.size - 1
    one[Hp - 1, Wp - 1] = -7.25                                               # ... and as the minimum
    be.setIG(one)
    out = be.publishEventImage(0.75)
    assert out[Hp - 1, Wp - 1] == 255 and (out == 0).sum() == out.size - 1

    V = dr.vote_image(Wp, Hp, 60_000, seed=Hp)
    be.setIG(V)
    for g in GAMMAS:
        mono = be.publishEventImage(g)
        dr.assert_levels(mono, dr.pano_levels(V, g), inverted=True, verbose="votes %dx%d gamma %.2f" % (Wp, Hp, g))
        bgr = be.publishEventImage(g, q)
        assert bgr.shape == (Hp, Wp, 3)
        assert (bgr[on] == (255, 0, 0)).all()
        np.testing.assert_array_equal(bgr[~on], dr.gray_to_bgr(mono)[~on])


# ------------------------------------------------------------------------------------------------ sensor outline
FOV_POSES = {
    "identity": (0.0, 0.0, 0.0, 1.0),
    "yaw across the seam": _qy(np.pi - 0.2),
    "pitch 60 deg": _qx(np.pi / 3),
    "pitch to the pole": _qx(np.radians(-65.9)),   # the outline's far edge rounds to row Hp: those points are skipped
}


@pytest.mark.parametrize("pose", list(FOV_POSES))
def test_fov_outline(hip, pose):
    W, H, Wp, Hp = 240, 180, 512, 256
    lut = synth.pinhole_lut(W, H, 200.0, 200.0, 119.5, 89.5)
    be = hip.BackendEvaluator(W, H, lut, Wp, Hp)
    V = dr.vote_image(Wp, Hp, 50_000, seed=17)
    be.setIG(V)
    q = FOV_POSES[pose]
    pix, tie = dr.fov_pixels(W, H, lut, q, Wp, Hp)
    assert tie > 1e-9, "a projected coordinate of this pose lies on a rounding tie: choose another pose"
    p = np.rint(dr.fov_projection(W, H, lut, q, Wp, Hp))
    skipped = int(((p[:, 0] < 0) | (p[:, 0] >= Wp) | (p[:, 1] < 0) | (p[:, 1] >= Hp)).sum())
    if pose in ("pitch to the pole", "yaw across the seam"):
        assert skipped > 0
    if pose == "yaw across the seam":
        xs = np.array(sorted(pix))[:, 0]
        assert xs.min() < 64 and xs.max() > Wp - 64
    mono = be.publishEventImage(0.75)
    bgr = be.publishEventImage(0.75, q)
    on = np.zeros((Hp, Wp), bool)
    on[[y for _, y in pix], [x for x, _ in pix]] = True
    changed = (bgr != dr.gray_to_bgr(mono)).any(axis=2)
    np.testing.assert_array_equal(changed, on)                # the set matches exactly, nothing else is written
    assert (bgr[on] == (255, 0, 0)).all()
    # an unnormalised quaternion names the same pose
    np.testing.assert_array_equal(be.publishEventImage(0.75, tuple(3.0 * v for v in q)), bgr)


# ------------------------------------------------------------------------------------------------ state is untouched
def test_frontend_state_untouched_deterministic(hip):
    p = _packet("240x180")
    om1, om2 = np.array([0.3, -0.5, 0.2]), np.asarray(p.omega_true, np.float64)

    def run(render, prepare):
        fe = hip.FrontendEvaluator(p.W, p.H, p.lut)
        fe.set_deterministic()
        _set_packet(fe, p)
        if prepare:
            fe.prepare(om1)
        res = []
        if render:
            fe.publishEventImage(om2)
        res.append(fe.eval(om1))
        if render:
            fe.publishEventImage(om1)     # the very point of the resident image: the next df must not reuse display planes
        res.append(fe.eval(om1))
        res.append(fe.eval(om2, False))
        if render:
            fe.publishEventImage(om2)
        res.append(fe.eval(om2))
        if render:
            fe.publishEventImage(np.zeros(3))
        x, rep = fe.setupProblemAndOptimize(np.zeros(3))
        if render:
            fe.publishEventImage(x)
        x2, rep2 = fe.setupProblemAndOptimize(np.zeros(3))
        return res, (x, rep), (x2, rep2)

    for prepare in (False, True):
        (r0, s0, s0b), (r1, s1, s1b) = run(False, prepare), run(True, prepare)
        for (c0, g0), (c1, g1) in zip(r0, r1):
            assert c0 == c1
            assert (g0 is None and g1 is None) or np.array_equal(g0, g1)
        for (xa, ra), (xb, rb) in ((s0, s0b), (s0, s1), (s0b, s1b), (s1, s1b)):
            np.testing.assert_array_equal(xa, xb)
            assert ra == rb


def _solve_render_solve(hip):
    p = _packet("240x180")
    fe = hip.FrontendEvaluator(p.W, p.H, p.lut)
    _set_packet(fe, p)
    x0, rep0 = fe.setupProblemAndOptimize(np.zeros(3))
    fe.publishEventImage(x0)
    x1, rep1 = fe.setupProblemAndOptimize(np.zeros(3))
    print("solve before / after a render:", x0, rep0, x1, rep1)
    assert fe.stats()["chain_solves"] == 2   # both solves ran device-driven
    return (x0, rep0), (x1, rep1)


def test_frontend_solve_after_render_production_final_cost(hip):
    """Without the option (the device-driven solve is only eligible there): a solve after a render reaches the final cost of
    the solve before it within RTOL.  Measured: 7.6e-10 .. 9.4e-9 over nine pairs."""
    (_, rep0), (_, rep1) = _solve_render_solve(hip)
    assert rel_scalar(rep1["final_cost"], rep0["final_cost"]) < RTOL


def test_frontend_solve_after_render_production_estimate(hip):
    """... and its estimate within RTOL.  THIS BOUND IS NOT MET, and not because of the render: on this packet the estimates of
    repeated production solves from the same start differ in max-norm, relative to the estimate, by
        1.9e-6 .. 4.3e-5  with nothing between the solves (nine pairs on three contexts; 1.1e-5 .. 2.5e-5 between fresh contexts),
        2.6e-6 .. 4.3e-5  with two cmx_frontend_get_iwe calls between them,
        8.7e-7 .. 3.4e-5  with a render between them,
    while the final costs agree to 1e-8: the votes are sums of fp32 atomics in arrival order, the line search takes 35, 38 or
    43 cost evaluations depending on their last bits, and the loose stopping rule (tolfun 1e-4) ends it at slightly different
    points of a flat optimum.  The test passes or fails with that noise (about every second run).  With
    CMX_OPT_DETERMINISTIC the solve after a render is bit-identical to the one before
    (test_frontend_state_untouched_deterministic)."""
    (x0, _), (x1, _) = _solve_render_solve(hip)
    assert rel_vec(x1, x0) < RTOL


def test_backend_state_untouched_deterministic(hip):
    w = synth.backend_window(40_003, 240, 180, 200.0, 200.0, 119.5, 89.5, 512, 256, 2, 5, 1, 0.2, seed=21)
    q = w.knots_true[2]

    def run(render):
        be = hip.BackendEvaluator(w.W, w.H, w.lut, w.Wp, w.Hp)
        be.set_deterministic()
        be.setIG(dr.vote_image(w.Wp, w.Hp, 20_000, seed=5))
        be.set_window(w.x, w.y, w.t_ns, 2, w.knots_init, w.start_ns, w.dt_ns, w.num_fixed, w.t_next_win_beg_ns, IG="resident")
        res = []
        for d in (np.zeros(w.P), np.full(w.P, 0.002)):
            if render:
                be.publishEventImage(0.75)
            res.append(be.eval(d))
            if render:
                be.publishEventImage(0.5, q)
            res.append(be.eval(d, False))
        be.updateIG(1)
        if render:
            be.publishEventImage(0.75, q)
        IG = be.getIG()
        if render:
            be.publishEventImage(1.0)
        res.append(be.eval(np.full(w.P, -0.001)))
        return res, IG

    (r0, IG0), (r1, IG1) = run(False), run(True)
    for (c0, g0), (c1, g1) in zip(r0, r1):
        assert c0 == c1
        assert (g0 is None and g1 is None) or np.array_equal(g0, g1)
    np.testing.assert_array_equal(IG0, IG1)


# ------------------------------------------------------------------------------------------------ errors
def test_display_errors(hip):
    L = _lib.lib()
    p = _packet("240x180")
    fe = hip.FrontendEvaluator(p.W, p.H, p.lut)
    be = hip.BackendEvaluator(p.W, p.H, p.lut, 256, 128)
    img = np.zeros((p.H, 2 * p.W), np.uint8)
    pano = np.zeros((128, 256, 3), np.uint8)
    o, po = img.ctypes.data_as(U8P), pano.ctypes.data_as(U8P)
    om = (C.c_double * 3)(0.1, 0.2, 0.3)
    q = (C.c_double * 4)(0.0, 0.0, 0.0, 1.0)
    zq = (C.c_double * 4)(0.0, 0.0, 0.0, 0.0)

    def expect(ctx, rc, code):
        assert rc == code, (rc, code)
        assert len(L.cmx_last_error(ctx)) > 0

    expect(fe._ctx, L.cmx_frontend_render_display(fe._ctx, om, o), _lib.ERR_STATE)          # before set_packet
    expect(be._ctx, L.cmx_frontend_render_display(be._ctx, om, o), _lib.ERR_STATE)          # wrong context kind
    expect(fe._ctx, L.cmx_backend_render_map(fe._ctx, 0.75, None, po), _lib.ERR_STATE)      # wrong context kind
    _set_packet(fe, p)
    expect(fe._ctx, L.cmx_frontend_render_display(fe._ctx, None, o), _lib.ERR_INVALID_ARG)
    expect(fe._ctx, L.cmx_frontend_render_display(fe._ctx, om, None), _lib.ERR_INVALID_ARG)
    expect(be._ctx, L.cmx_backend_render_map(be._ctx, 0.75, None, None), _lib.ERR_INVALID_ARG)
    for g in (0.0, -1.0, float("nan"), float("inf")):
        expect(be._ctx, L.cmx_backend_render_map(be._ctx, g, None, po), _lib.ERR_INVALID_ARG)
    expect(be._ctx, L.cmx_backend_render_map(be._ctx, 0.75, zq, po), _lib.ERR_INVALID_ARG)
    assert not img.any() and not pano.any()                                                  # nothing was written
    # both contexts survive all of the above
    assert L.cmx_frontend_render_display(fe._ctx, om, o) == _lib.OK and img.max() == 255
    assert L.cmx_backend_render_map(be._ctx, 0.75, q, po) == _lib.OK and pano.max() == 255
    c, g = fe.eval((0.1, 0.2, 0.3))
    assert np.isfinite(c) and np.all(np.isfinite(g))


# ------------------------------------------------------------------------------------------------ group
def test_group_renders_member_zero(hip):
    W, H, Wp, Hp = 240, 180, 512, 256
    lut = synth.pinhole_lut(W, H, 200.0, 200.0, 119.5, 89.5)
    grp = hip.BackendEvaluator(W, H, lut, Wp, Hp, devices=[0, 0])
    one = hip.BackendEvaluator(W, H, lut, Wp, Hp)
    V = dr.vote_image(Wp, Hp, 50_000, seed=23)
    q = _qx(np.pi / 3)
    for e in (grp, one):
        e.setIG(V)
    np.testing.assert_array_equal(grp.publishEventImage(0.75), one.publishEventImage(0.75))
    np.testing.assert_array_equal(grp.publishEventImage(2.2, q), one.publishEventImage(2.2, q))
    dr.assert_levels(grp.publishEventImage(0.75), dr.pano_levels(V, 0.75), inverted=True)
    for e in (grp, one):
        e.close()


# ------------------------------------------------------------------------------------------------ example
def test_example_writes_display_images(hip, tmp_path):
    import os
    import sys
    ex = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples")
    if ex not in sys.path:
        sys.path.insert(0, ex)
    import rotation_pipeline as rp
    stream = synth.event_stream(2e6, 0.5, 240, 180, 200.0, 200.0, 119.5, 89.5, omega_mean=(0.2, 1.8, 0.3),
                                omega_amp=(1.0, 0.8, 1.0), seed=77)
    prm = rp.Params()
    res = rp.run_pipeline(stream, prm, display_prefix=str(tmp_path / "shot"))
    Hp, Wp = res["IG"].shape
    pgm = (tmp_path / "shot_local_iwe.pgm").read_bytes()
    ppm = (tmp_path / "shot_pano.ppm").read_bytes()
    head = b"P5\n%d %d\n255\n" % (2 * stream.W, stream.H)
    assert pgm.startswith(head) and len(pgm) == len(head) + 2 * stream.W * stream.H
    head = b"P6\n%d %d\n255\n" % (Wp, Hp)
    assert ppm.startswith(head) and len(ppm) == len(head) + 3 * Wp * Hp
    rgb = np.frombuffer(ppm[len(head):], np.uint8).reshape(Hp, Wp, 3)
    outline = (rgb == (0, 0, 255)).all(axis=2)            # (B, G, R) = (255, 0, 0) is blue; the file is RGB
    assert 100 < outline.sum() <= 2 * (stream.W + stream.H)
    grey = (rgb[..., 0] == rgb[..., 1]) & (rgb[..., 1] == rgb[..., 2])
    np.testing.assert_array_equal(grey, ~outline)
    mono = 255 - rgb[..., 0][grey].astype(np.int64)
    assert mono.max() == 255 and (mono > 0).mean() > 0.02
