"""CPU: conditions on the cases of the map-upkeep tests (tests/map_cases.py), so that the GPU tests cannot pass emptily.  Needs no GPU.

Every figure a guard rests on is printed before it is asserted (pytest -s shows them): the distance of the projected sensor pixels
to the nearest integer, the edge-column and edge-row counts of every footprint, the cells the reference's row test removes, and
what rounding, the transposed rotation and the upper part of a large sensor change."""
import numpy as np
import pytest

import map_cases as mc
from oracle import iwe_numpy

GUARDED = tuple(sorted(set(mc.FOOTPRINTS) | {(g, mc.second_pose(g, p)) for g, p in mc.FOOTPRINTS}
                       | {(mc.SEQUENCE[0], p) for p in mc.SEQUENCE[1]} | {("p512", p) for p, _ in mc.PARTNERS.values()}))


def _dims(geom):
    g = mc.GEOMS[geom]
    return g["W"], g["H"], g["Wp"], g["Hp"]


def test_case_table_is_the_one_the_tests_describe():
    assert {g: (v["W"], v["H"], v["f"], v["Wp"], v["Hp"]) for g, v in mc.GEOMS.items() if g != "general"} == {
        "p512": (240, 180, 200.0, 512, 256), "p130": (240, 180, 200.0, 130, 96), "p64": (64, 48, 50.0, 64, 32),
        "p1000": (640, 480, 500.0, 1000, 300), "p2048": (240, 180, 200.0, 2048, 1024)}
    for g in mc.GEOMS:
        assert set(mc.GEOM_RADII[g]) >= {0, 1, 3}
        for p in mc.GEOM_POSES[g]:
            assert mc.second_pose(g, p) != p
    print("%d footprints (geometry, pose), %d cases with their radii" % (len(mc.FOOTPRINTS), len(mc.CASES)))
    assert ("p64", "mid", 64) in mc.CASES and ("p130", "north", 7) in mc.CASES and ("p1000", "south", 0) in mc.CASES
    assert {p for g, p, _ in mc.CASES if g == "p2048"} == {"mid", "seam"} and len(set(mc.CASES)) == len(mc.CASES)
    assert 7 in mc.GEOM_RADII["p130"] and 64 in mc.GEOM_RADII["p64"]
    assert [g for g in mc.GEOMS if 64 in mc.GEOM_RADII[g]] == ["p64"]        # the API's maximum, on the smallest panorama only
    assert (130 * 96) % 256 != 0
    assert 240 * 180 < mc.MARK_LANES < 640 * 480                            # only p1000 takes a second step of the mark kernel
    assert 1000 * 300 < mc.UPDATE_LANES < 2048 * 1024                       # only p2048 takes one of the update / add kernels
    assert not np.all(mc.lut("general").reshape(-1, 3)[:, 2] == 1.0) and np.all(mc.lut("p512").reshape(-1, 3)[:, 2] == 1.0)


def test_quaternion_is_the_rotation():
    for name, ypr in mc.POSES.items():
        q = mc.quat_ypr(*ypr)
        assert abs(np.linalg.norm(q) - 1) < 1e-15
        R = mc.rotation(*ypr)
        assert np.abs(iwe_numpy.q_to_R(q) - R).max() < 1e-15 and np.abs(R - R.T).max() > 1e-2, name


@pytest.mark.parametrize("geom,pose", GUARDED)
def test_exactness_guard(geom, pose):
    """no projected coordinate within GUARD of an integer, no ray on the seam's half plane or at a pole: the cell of every sensor
    pixel is the same under any fp64 atan2 / asin"""
    px, py = mc.project(geom, pose)
    v = mc.rays(geom, pose)
    d = mc.integer_distance(px, py)
    behind = v[:, 2] < 0
    on_seam = float(np.abs(v[behind, 0]).min()) if behind.any() else np.inf
    to_pole = float(1.0 - (np.abs(v[:, 1]) / np.sqrt((v * v).sum(axis=1))).max())
    print("%s/%s: min distance to an integer %.2e px, min |x| behind the camera %.2e, min 1 - |sin(latitude)| %.2e"
          % (geom, pose, d, on_seam, to_pole))
    _, _, Wp, Hp = _dims(geom)
    assert d >= mc.GUARD
    assert on_seam > 1e-9 and to_pole > 1e-9
    assert np.abs(px).max() <= 2048 and np.abs(py).max() <= 2048
    assert 0 < px.min() and px.max() < Wp and 0 < py.min() and py.max() < Hp


@pytest.mark.parametrize("geom,pose", mc.FOOTPRINTS)
def test_the_oracles_agree_and_the_footprint_is_where_it_should_be(oracle, geom, pose):
    W, H, Wp, Hp = _dims(geom)
    q = mc.quat(pose)
    for r in mc.GEOM_RADII[geom]:
        m = mc.mask(geom, pose, r)
        ref = oracle.Backend(W, H, mc.lut(geom), Wp, Hp, 2)
        ref.mark_visited(q, r)
        ut = np.zeros((Hp, Wp), np.uint8)
        iwe_numpy.mark_visited(ut, q, mc.lut(geom), W, H, Wp, Hp, r)
        np.testing.assert_array_equal(ref.update_times, ut)     # oracle/backend.c against oracle/iwe_numpy.py
        np.testing.assert_array_equal(ut, m)                    # ... and the restatement of map_cases
        col0, colW, row0, rowH = int(m[:, 0].sum()), int(m[:, -1].sum()), int(m[0].sum()), int(m[-1].sum())
        quirk = int((m != mc.mask(geom, pose, r, quirk=False)).sum())
        print("%s/%s r=%d: %d cells; column 0 / Wp-1: %d / %d; row 0 / Hp-1: %d / %d; removed by the row test: %d"
              % (geom, pose, r, int(m.sum()), col0, colW, row0, rowH, quirk))
        assert 0 < m.sum() < m.size or r == 64
        if r > 7:
            continue        # (radius 64 covers a 64 x 32 panorama's every column: the conditions below are about footprints)
        if pose in ("seam", "seam_neg", "left"):
            assert col0 > 0 and colW > 0
        if pose == "north":
            assert row0 > 0 and rowH == 0
        if pose == "south":
            assert rowH > 0 and row0 == 0
        if pose == "mid":
            assert col0 == colW == row0 == rowH == 0
        if geom in ("p512", "p1000", "general"):
            if pose == "north" and r in (1, 3):
                assert quirk > 0
            if pose != "north":
                assert quirk == 0


@pytest.mark.parametrize("geom", [g for g in mc.GEOMS if "north" in mc.GEOM_POSES[g]])
def test_one_cell_mistakes_show_at_radius_0(geom):
    m = mc.mask(geom, "north", 0)
    rounded = int((m != mc.mask(geom, "north", 0, rounding=True)).sum())
    transposed = int((m != mc.mask(geom, "north", 0, transpose=True)).sum())
    holes = int((m[:m.shape[0] // 4] == 0).sum())
    print("%s/north r=0: %d cells differ with rounding, %d with the transposed rotation; %d unmarked cells in the top quarter"
          % (geom, rounded, transposed, holes))
    assert rounded > 0 and transposed > 0 and holes > 0


@pytest.mark.parametrize("geom,pose", [(g, p) for g, p in mc.FOOTPRINTS if g != "general"])
def test_rounding_and_transpose_show_on_every_pose(geom, pose):
    m = mc.mask(geom, pose, 0)
    rounded = int((m != mc.mask(geom, pose, 0, rounding=True)).sum())
    transposed = int((m != mc.mask(geom, pose, 0, transpose=True)).sum())
    print("%s/%s r=0: rounding changes %d cells, the transposed rotation %d" % (geom, pose, rounded, transposed))
    assert rounded > 0 and transposed > 0


@pytest.mark.parametrize("pose", mc.GEOM_POSES["p1000"])
def test_upper_sensor_pixels_mark_cells_of_their_own(pose):
    """640 x 480: the sensor pixels past the first step of the mark kernel's grid mark cells nobody else marks"""
    W, H, _, _ = _dims("p1000")
    assert W * H > mc.MARK_LANES
    first = np.arange(W * H) < mc.MARK_LANES
    own = int(((mc.mask("p1000", pose, 0) == 1) & (mc.mask("p1000", pose, 0, pixels=first) == 0)).sum())
    print("p1000/%s r=0: %d cells marked only by sensor pixels with index >= %d" % (pose, own, mc.MARK_LANES))
    assert own > 0


def test_wrapping_the_column_would_show():
    """a kernel that wrapped the column at the seam would mark a superset of the mask, and on `left` (a rolled footprint whose
    corner alone crosses column 0) strictly more"""
    for geom in ("p512", "p130", "p64", "p1000"):
        _, _, Wp, Hp = _dims(geom)
        for pose in ("seam", "seam_neg", "left"):
            ic, ir = mc.cells(geom, pose)
            m = mc.mask(geom, pose, 3)
            wrapped = np.zeros_like(m)
            for dj in range(-3, 4):
                for di in range(-3, 4):
                    ym = ir + dj
                    ok = (0 <= ym + dj) & (ym < Hp) & (ym >= 0)
                    wrapped[ym[ok], (ic[ok] + di) % Wp] = 1
            extra = int((wrapped != m).sum())
            print("%s/%s r=3: wrapping the column would mark %d more cells" % (geom, pose, extra))
            assert not (m & ~wrapped).any()
            if pose == "left":   # (a footprint that straddles the seam is contiguous across it: wrapping may add nothing there)
                assert extra > 0


@pytest.mark.parametrize("geom,pose", [("p512", "seam"), ("p512", "north"), ("p130", "mid"), ("p130", "seam_neg")])
def test_windows_seen_from_a_pose(oracle, geom, pose):
    """the windows of the evaluation tests: the scene lies around the pose, and the count of votes the sum test of the GPU tests
    uses is the oracle's own IL_old.sum()"""
    W, H, Wp, Hp = _dims(geom)
    w = mc.window(geom, pose)
    ref = oracle.Backend(W, H, mc.lut(geom), Wp, Hp, 2)
    ref.set_window(w.x, w.y, w.t_ns, w.knots_init, w.start_ns, w.dt_ns, w.num_fixed, w.t_next_win_beg_ns)
    d = 0.004 * np.sin(np.arange(w.P) + 1.0)
    ref.eval(d, False)
    knots = oracle.left_update(w.knots_init, d, w.num_fixed)
    n = mc.old_votes_inside(w, mc.lut(geom), lambda t: oracle.spline_eval(2, knots, w.start_ns, w.dt_ns, t, jac=False)[1])
    s = float(ref.IL_old.sum(dtype=np.float64))
    print("%s/%s: %d of %d events vote into IL_old, IL_old.sum() = %.6f" % (geom, pose, n, len(w.x), s))
    assert 0.2 * len(w.x) < n < len(w.x) and abs(s - n) < 1e-5 * n
    if pose in ("seam", "seam_neg"):
        assert ref.IL_old[:, :8].any() and ref.IL_old[:, -8:].any() and not ref.IL_old[:, Wp // 2 - 8:Wp // 2 + 8].any()
    if pose == "north":
        assert ref.IL_old[:8].any() and not ref.IL_old[Hp // 2:].any()
