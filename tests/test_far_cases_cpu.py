"""No GPU: what tests/test_gpu_far_orientations.py takes for granted about tests/far_cases.py.

Probe tables: the CPU oracle's own vote loop puts every probe where probe_reference says (so a per-event difference found on the
device is the device's), both sides of the border rule are populated at all four borders, and no probe sits so close to an integer
pixel coordinate that a last-place difference in atan2 / asin could move it to another cell.
Far windows: the oracle is within 2e-6 of the exact (fp64) arithmetic there, so its own fp32 rounding leaves the 1e-5 bar of the
GPU tests meaningful at the seam and at the poles; at least 85 % of the events vote; and the 30-degree pitch really has rays on
both sides of |sin(theta)| = 1/2 inside one wave's 64 consecutive events (lean_asin's wave-uniform branch with mixed lanes)."""
import numpy as np
import pytest

import far_cases as fc
from util import rel_scalar, rel_vec


@pytest.fixture(scope="module", autouse=True)
def _oracle(oracle):
    return oracle


def _oracle_planes(oracle, tab, old):
    ref = oracle.Backend(fc.SENSOR, fc.SENSOR, tab.lut, tab.Wp, tab.Hp, 2, fc.BATCH, 1, 0.0, 0)
    start_ns, dt_ns, t_next = tab.window_args(old)
    ref.set_window(tab.x, tab.y, tab.t_ns, tab.knots, start_ns, dt_ns, 1, t_next)
    il_old, il_new, _ = ref.accumulate_raw(np.zeros(3))
    return il_old.copy(), il_new.copy()


@pytest.mark.parametrize("Wp,Hp", fc.PANOS)
@pytest.mark.parametrize("name,z1", fc.PROBE_CASES)
def test_probe_table_against_the_oracle(oracle, Wp, Hp, name, z1):
    tab, ref = fc.probe_case(Wp, Hp, name, z1)       # (probe_reference asserts disjoint cells and the distance >= 1e-7)
    assert tab.n % fc.BATCH != 1 and len(tab.lut) == fc.N_PROBES and (tab.n == fc.N_PROBES or (z1 and Wp == 512))
    assert np.all(tab.lut[:, 2] == 1.0) if z1 else (tab.lut[:, 2] < 0).any() and (tab.lut[:, 2] > 0).any()
    n_kept, n_drop = int(ref.kept.sum()), int((~ref.kept).sum())
    for old in (True, False):
        il_old, il_new = _oracle_planes(oracle, tab, old)
        mine, other = (il_old, il_new) if old else (il_new, il_old)
        worst = fc.compare_plane(tab, ref, tab.Q.as_matrix(), mine, 4e-7)
        assert not other.any()
        assert abs(float(mine.sum(dtype=np.float64)) - n_kept) < 1e-5
    left, right = ref.xx < 1, ref.xx >= Wp - 2
    top, bottom = ref.yy < 1, ref.yy >= Hp - 2
    reg = ~tab.is_pole
    sides = [int((s & reg).sum()) for s in (left, right, top, bottom)]
    print("%dx%d %s%s: %d kept / %d dropped (left %d right %d top %d bottom %d), min distance %.2e, oracle max difference %.2e"
          % (Wp, Hp, name, " z1" if z1 else "", n_kept, n_drop, *sides, ref.dist[reg].min(), worst))
    if not z1:
        assert n_kept >= 50 and n_drop >= 50
        assert min(sides) > 0, sides
    elif name == "identity":
        # 75 degrees around +z reaches neither the seam nor a pole row: every probe is kept (the z = 1 load and rotation
        # are what this table is for; its borders are the general table's)
        assert n_drop == 0 and tab.n_pole == 0 and n_kept >= 2000
    else:
        # a camera looking at a pole: that pole's rows and the seam columns next to it, and the pole itself
        assert n_kept >= 50 and n_drop >= 50 and tab.n_pole == 1
        assert sides[0] > 0 and sides[1] > 0 and max(sides[2], sides[3]) > 0 and min(sides[2], sides[3]) == 0


def test_probe_table_is_reproducible():
    a = fc.probe_table(512, 256, fc.PROBE_ORIENTATIONS["general"], 11)
    b = fc.probe_table(512, 256, fc.PROBE_ORIENTATIONS["general"], 11)
    assert np.array_equal(a.lut, b.lut)
    n = np.linalg.norm(a.lut, axis=1)
    assert n.min() < 0.7 and n.max() > 2.5          # |b| != 1: the rho normalisation matters
    special = np.isin(np.round(a.target[:-2] % 1.0, 9), [1e-6, 1 - 1e-6, 0.5]).any(axis=1)
    assert 0.1 < special.mean() < 0.3               # a tenth per axis
    assert (a.target[:-2, 0] >= 508).sum() >= 10 and (a.target[:-2, 1] >= 252).sum() >= 10


@pytest.mark.parametrize("which,name", fc.FAR_CASES)
@pytest.mark.parametrize("measure", [0, 1])
def test_far_window_oracle_against_exact(oracle, which, name, measure):
    w = fc.far_window(which, name)
    args = (w.W, w.H, w.lut, w.Wp, w.Hp, w.order, w.batch, w.sample_rate, w.sigma, measure)
    win = (w.x, w.y, w.t_ns, w.knots_init, w.start_ns, w.dt_ns, w.num_fixed, w.t_next_win_beg_ns)
    ref, ex = oracle.Backend(*args), oracle.BackendExact(*args)
    ref.set_window(*win)
    ex.set_window(*win)
    for d in fc.far_points(w):
        (c, g), (ce, ge) = ref.eval(d), ex.eval(d)
        print("%s %s measure %d: oracle vs exact contrast %.2e gradient %.2e" % (which, name, measure, rel_scalar(c, ce), rel_vec(g, ge)))
        assert rel_scalar(c, ce) < 2e-6 and rel_vec(g, ge) < 2e-6
    il_old, il_new, _ = ref.accumulate_raw(np.zeros(w.P))
    votes = float(il_old.sum(dtype=np.float64) + il_new.sum(dtype=np.float64))
    print("%s %s: %.0f / %d events vote" % (which, name, votes, len(w.x)))
    assert votes >= 0.85 * len(w.x)
    assert il_old.sum() > 0 and il_new.sum() > 0


def test_rotated_turns_the_scene_with_the_camera():
    w0 = fc.base_window("linear")
    w = fc.far_window("linear", "yaw180")
    assert w.x is w0.x and w.t_ns is w0.t_ns
    r0, r = fc.world_rays(w0), fc.world_rays(w)
    assert np.abs(r - fc.FAR["yaw180"].apply(r0)).max() < 1e-12
    assert np.median(r0[:, 2]) > 0.9 and np.median(r[:, 2]) < -0.9     # behind the panorama's centre: at the +-pi seam
    assert (r[:, 0] > 0).mean() > 0.2 and (r[:, 0] < 0).mean() > 0.2   # ... on both sides of it


def test_far_windows_reach_what_they_are_for():
    for which in ("linear", "cubic"):
        s = np.abs(fc.world_rays(fc.far_window(which, "pitch30"))[:, 1])
        big = s > 0.5
        assert 0.2 < big.mean() < 0.8
        runs = big[:len(big) // 64 * 64].reshape(-1, 64)     # a wave of the reference-shaped splat: 64 consecutive events
        mixed = runs.any(axis=1) & ~runs.all(axis=1)
        assert mixed.mean() > 0.9
    for name in ("pitch80", "pitch-80", "pitch90"):
        r = fc.world_rays(fc.far_window("linear", name))
        assert (np.abs(r[:, 1]) > np.sin(np.deg2rad(80))).mean() > 0.1    # a tenth of the rays within 10 degrees of a pole
    r = fc.world_rays(fc.far_window("linear", "pitch90"))
    assert (np.abs(r[:, 2]) > np.abs(r[:, 0])).any() and (np.abs(r[:, 0]) > np.abs(r[:, 2])).any() and (r[:, 2] < 0).any()
