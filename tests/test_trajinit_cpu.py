"""CPU tests for the control-pose initialisation: host C++ behind the C ABI
(csrc/cmx_trajinit.cpp) against the oracle (oracle/traj_init.c), the oracle against vectors produced by the
reference's vendored Eigen / Sophus (tests/golden/trajinit.npz), and size-independent properties."""
import os

import numpy as np
import pytest

from cmax_slam_amd import _lib, synth, trajectory
from oracle import pyoracle as po

G = np.load(os.path.join(os.path.dirname(__file__), "golden", "trajinit.npz"))
T0 = 1_000_000_000


# ----------------------------------------------------------------------------- oracle pinned by the reference
def test_oracle_qr_matches_vendored_eigen_vectors():
    for A, b, x, (r, c), rank in zip(G["qr_A"], G["qr_b"], G["qr_x"], G["qr_shape"], G["qr_rank"]):
        xo, ro = po.fullpiv_qr_solve(A[:r, :c], b[:r])
        assert ro == rank
        np.testing.assert_allclose(xo, x[:c], rtol=0, atol=1e-12 * max(1.0, np.abs(x).max()))
    assert (G["qr_rank"] < G["qr_shape"][:, 1]).sum() >= 5  # rank-deficient systems are in the set


def test_oracle_so3_product_matches_vendored_sophus_vectors():
    for a, b, ab in zip(G["mul_a"], G["mul_b"], G["mul_ab"]):
        np.testing.assert_allclose(po.so3_mul(a, b), ab, rtol=0, atol=1e-15)


def test_oracle_qr_matches_live_eigen():
    """100 seeded random systems (dense, a zero column, 60 % zeros): the oracle against Eigen's solutions and ranks recorded in
    ref_random_cases.npz (oracle/gen_golden.py), and against the compiled reference itself where oracle/_ref is built."""
    rc = np.load(os.path.join(os.path.dirname(__file__), "golden", "ref_random_cases.npz"))
    live = po.ref_lib() is not None
    assert len(rc["qr_rank"]) == 100
    for Ap, bp, xp, (r, c), rank in zip(rc["qr_A"], rc["qr_b"], rc["qr_x"], rc["qr_shape"], rc["qr_rank"]):
        A, b = Ap[:r, :c], bp[:r]
        refs = [(xp[:c], int(rank))]
        if live:
            refs.append(po.fullpiv_qr_solve(A, b, use_ref=True))
        x1, k1 = po.fullpiv_qr_solve(A, b)
        for x0, k0 in refs:
            assert k0 == k1
            np.testing.assert_allclose(x1, x0, rtol=0, atol=1e-12 * max(1.0, np.abs(x0).max()))


def test_oracle_regression_vectors():
    for order, tag in ((2, "lin"), (4, "cub")):
        n = po.num_ctrl_poses(order, T0, T0 + 200_000_000, 0.05)
        assert n == int(G[tag + "_num_cps"]) == (5 if order == 2 else 7)  # launch defaults (SURVEY B-note)
        cps = po.fit_ctrl_poses(order, G[tag + "_pose_t"], G[tag + "_pose_q"], 1.0, 0.05, n)
        np.testing.assert_allclose(cps, G[tag + "_cps"], rtol=0, atol=1e-13)
    pt, pq, _, _ = po.integrate_ang_vel(G["iav_t"], G["iav_w"], T0, po.so3_exp([0, np.pi / 2, 0]), T0, G["iav_w"][0], True)
    assert np.array_equal(pt, G["iav_pose_t"])
    np.testing.assert_allclose(pq, G["iav_pose_q"], rtol=0, atol=1e-15)
    np.testing.assert_allclose(po.bearing_lut(64, 48, G["lut_K"], G["lut_D"]), G["lut_64x48"], rtol=0, atol=1e-15)


# ----------------------------------------------------------------------------- product (C ABI) vs oracle
def test_integrate_ang_vel_matches_oracle_and_golden():
    q0 = po.so3_exp([0, np.pi / 2, 0])
    (pt, pq), prev = trajectory.integrateAngVel((T0, q0), (G["iav_t"], G["iav_w"]), (T0, G["iav_w"][0]), True)
    assert np.array_equal(pt, G["iav_pose_t"])
    np.testing.assert_allclose(pq, G["iav_pose_q"], rtol=0, atol=1e-15)
    assert prev[0] == G["iav_t"][-1] and np.array_equal(prev[1], G["iav_w"][-1])
    # second window: stamps not newer than ang_vel_prev_ are skipped, state carries over
    t2 = np.concatenate([G["iav_t"][-2:], G["iav_t"][-1] + 10_000_000 * np.arange(1, 6)])
    w2 = np.vstack([G["iav_w"][-2:], G["iav_w"][:5]])
    (pt2, pq2), prev2 = trajectory.integrateAngVel((int(pt[-1]), pq[-1]), (t2, w2), prev, False)
    ot, oq, ot_prev, ow_prev = po.integrate_ang_vel(t2, w2, int(pt[-1]), pq[-1], prev[0], prev[1], False)
    assert len(pt2) == 5 and np.array_equal(pt2, ot) and prev2[0] == ot_prev
    np.testing.assert_allclose(pq2, oq, rtol=0, atol=1e-15)


def test_integrate_constant_rate_is_exact_rotation():
    w = np.array([0.6, -0.9, 0.4])
    t = T0 + 10_000_000 * np.arange(1, 41, dtype=np.int64)
    (pt, pq), _ = trajectory.integrateAngVel((T0, [0, 0, 0, 1.0]), (t, np.tile(w, (40, 1))), (T0, w), True)
    expect = po.so3_exp(w * 0.4)
    assert min(np.abs(pq[-1] - expect).max(), np.abs(pq[-1] + expect).max()) < 1e-12


@pytest.mark.parametrize("degree", [1, 3])
def test_fit_ctrl_poses_matches_oracle(degree):
    rng = np.random.default_rng(17 + degree)
    order = 2 if degree == 1 else 4
    for trial in range(20):
        step = int(rng.choice([10_000_000, 5_000_000, 20_000_000]))
        span = 200_000_000 if trial % 2 == 0 else 100_000_000
        n = span // step
        t = T0 + step // 2 + step * np.arange(n, dtype=np.int64)
        q = np.array([po.so3_exp(v) for v in np.cumsum(rng.normal(0, 0.02, (n, 3)), axis=0) + rng.normal(0, 1, 3)])
        traj = trajectory.Trajectory(degree, T0, 0.05)
        if n < po.num_ctrl_poses(order, T0, T0 + span, 0.05):
            with pytest.raises(trajectory.CmaxHipError):
                traj.generateCtrlPoses((t, q), T0, T0 + span)
            continue
        cps = traj.generateCtrlPoses((t, q), T0, T0 + span)
        ref = po.fit_ctrl_poses(order, t, q, 1.0, 0.05, po.num_ctrl_poses(order, T0, T0 + span, 0.05))
        np.testing.assert_allclose(cps, ref, rtol=0, atol=1e-12)
    for tag, o in (("lin", 2), ("cub", 4)):  # golden
        if o != order:
            continue
        traj = trajectory.Trajectory(degree, T0, 0.05)
        cps = traj.generateCtrlPoses((G[tag + "_pose_t"], G[tag + "_pose_q"]), T0, T0 + 200_000_000)
        np.testing.assert_allclose(cps, G[tag + "_cps"], rtol=0, atol=1e-12)


@pytest.mark.parametrize("degree", [1, 3])
def test_fit_recovers_a_curve_that_is_a_bspline_in_the_tangent_space(degree):
    """If log(offset^-1 R(t)) is exactly a uniform B-spline of the control vectors, the fit returns them."""
    rng = np.random.default_rng(3)
    order = 2 if degree == 1 else 4
    ncp = 5 if degree == 1 else 7
    M = (np.array([[1.0, 0.0], [-1.0, 1.0]]) if degree == 1 else
         np.array([[1 / 6, 2 / 3, 1 / 6, 0], [-0.5, 0, 0.5, 0], [0.5, -1, 0.5, 0], [-1 / 6, 0.5, -0.5, 1 / 6]]))
    P = rng.normal(0, 0.2, (ncp, 3))
    t = T0 + 2_500_000 + 5_000_000 * np.arange(40, dtype=np.int64)
    tang = []
    for ti in t:
        s = (ti - T0) * 1e-9 / 0.05
        seg = int(np.floor(s)); u = s - seg
        tang.append((u ** np.arange(order)) @ M @ P[seg:seg + order])
    tang = np.array(tang)
    # partition of unity: shifting every control vector by -tang[0] shifts the curve by -tang[0], so the curve
    # passes through 0 at the first sample and the first pose IS the offset the fit lifts with
    P = P - tang[0]
    tang = tang - tang[0]
    offset = po.so3_exp([0.3, -1.2, 0.5])
    q = np.array([po.so3_mul(offset, po.so3_exp(v)) for v in tang])
    cps = trajectory.Trajectory(degree, T0, 0.05).generateCtrlPoses((t, q), T0, T0 + 200_000_000)
    expect = np.array([po.so3_mul(offset, po.so3_exp(v)) for v in P])
    np.testing.assert_allclose(cps, expect, rtol=0, atol=1e-9)


def test_rank_deficient_fit_matches_oracle():
    """All poses in the first segment: later control poses are unsupported -> Eigen's basic solution (zeros)."""
    rng = np.random.default_rng(9)
    t = T0 + 1_000_000 + 4_000_000 * np.arange(10, dtype=np.int64)  # all inside [0, 0.05)
    q = np.array([po.so3_exp(v) for v in np.cumsum(rng.normal(0, 0.01, (10, 3)), axis=0)])
    for degree, order in ((1, 2), (3, 4)):
        n = po.num_ctrl_poses(order, T0, T0 + 200_000_000, 0.05)
        cps = trajectory.Trajectory(degree, T0, 0.05).generateCtrlPoses((t, q), T0, T0 + 200_000_000)
        np.testing.assert_allclose(cps, po.fit_ctrl_poses(order, t, q, 1.0, 0.05, n), rtol=0, atol=1e-12)
        np.testing.assert_allclose(cps[-1], q[0], rtol=0, atol=1e-12)  # unsupported: increment zero -> the offset pose


def test_trajectory_update_and_evaluate_match_oracle():
    rng = np.random.default_rng(4)
    for degree, order in ((1, 2), (3, 4)):
        traj = trajectory.Trajectory(degree, T0, 0.05)
        traj.pushbackCtrlPoses([po.so3_exp(v) for v in np.cumsum(rng.normal(0, 0.05, (8, 3)), axis=0)])
        drot = rng.normal(0, 0.02, (5, 3))
        ref = po.left_update(traj.knots, drot, 3)
        traj.incrementalUpdate(drot, 3)
        np.testing.assert_allclose(traj.knots, ref, rtol=0, atol=1e-15)
        for t in (T0, T0 + 12_345_678, T0 + (8 - order + 1) * 50_000_000 - 1):
            q = traj.evaluate(t)
            qo, _, _, _ = po.spline_eval(order, traj.knots, T0, 50_000_000, t, jac=False)
            np.testing.assert_allclose(q, qo, rtol=0, atol=1e-14)
        with pytest.raises(trajectory.CmaxHipError):
            traj.evaluate(T0 + (8 - order + 1) * 50_000_000)  # Basalt would assert
        with pytest.raises(trajectory.CmaxHipError):
            traj.incrementalUpdate(drot, 2)                   # CHECK_EQ(idx_beg + drotv.size(), size())
        knots, start_ns, dt_ns = traj.temp_window(2)
        assert len(knots) == 6 and dt_ns == 50_000_000 and start_ns == po.traj_temp_start_ns(1.0, 2, 0.05)


def test_bearing_lut():
    K = np.array([[588.10, 0, 339.83], [0, 593.99, 242.43], [0, 0, 1.0]])
    lut = trajectory.bearing_lut(64, 48, K)
    np.testing.assert_array_equal(lut, synth.pinhole_lut(64, 48, 588.10, 593.99, 339.83, 242.43).reshape(48, 64, 3))
    np.testing.assert_allclose(trajectory.bearing_lut(64, 48, G["lut_K"], G["lut_D"]), G["lut_64x48"], rtol=0, atol=1e-15)
    # property: pushing the undistorted bearing back through the plumb_bob model lands on the raw pixel
    Ks, D = G["lut_K"], G["lut_D"]
    lut = trajectory.bearing_lut(64, 48, Ks, D)
    x, y = lut[..., 0], lut[..., 1]
    r2 = x * x + y * y
    rad = 1 + D[0] * r2 + D[1] * r2 ** 2 + D[4] * r2 ** 3
    xd = x * rad + 2 * D[2] * x * y + D[3] * (r2 + 2 * x * x)
    yd = y * rad + D[2] * (r2 + 2 * y * y) + 2 * D[3] * x * y
    u, v = Ks[0, 0] * xd + Ks[0, 2], Ks[1, 1] * yd + Ks[1, 2]
    uu, vv = np.meshgrid(np.arange(64.0), np.arange(48.0))
    inner = (slice(8, 40), slice(8, 56))
    assert np.abs(u - uu)[inner].max() < 0.05 and np.abs(v - vv)[inner].max() < 0.05
    with pytest.raises(trajectory.CmaxHipError):
        trajectory.bearing_lut(0, 48, K)


def test_time_order_is_enforced():
    t = np.array([T0 + 10, T0 + 5], np.int64)
    with pytest.raises(trajectory.CmaxHipError) as e:
        trajectory.integrateAngVel((T0, [0, 0, 0, 1.0]), (t, np.zeros((2, 3))), (T0, np.zeros(3)), True)
    assert e.value.status == _lib.ERR_TIME_ORDER
