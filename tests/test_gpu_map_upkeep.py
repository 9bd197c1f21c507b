"""-m gpu: device-resident global-map upkeep (EventWarper::updateIG / setUpdateTimesIG, event_pano_warper.cpp:81-126)
against the oracle, over a two-window sequence: solve window 1, fold IL_old into IG where the visit count allows,
mark the visited area, then evaluate window 2 against the RESIDENT map (CMX_KEEP_MAP) -- alpha and contrast must match
an oracle that carried the same map on the host.

Below the two sequence tests: the upkeep kernels themselves on the cases of tests/map_cases.py -- footprints cell for cell at the
seam, the poles and the borders, saturation, the update gate bit for bit, every way to arrive at updateIG, resident maps handed to
the next window, a four-window sequence, status codes.  Every figure is printed before it is asserted (-s)."""
import numpy as np
import pytest

from cmax_slam_amd import _lib, synth
from oracle import iwe_numpy
from util import RTOL, rel_img, rel_scalar, rel_vec

import map_cases as mc

pytestmark = pytest.mark.gpu


def test_two_windows_with_resident_map(hip, oracle):
    w1 = synth.backend_window(40_003, 240, 180, 200.0, 200.0, 119.5, 89.5, 512, 256, 2, 5, 1, 0.2, seed=21)
    w2 = synth.backend_window(40_003, 240, 180, 200.0, 200.0, 119.5, 89.5, 512, 256, 2, 5, 0, 0.2, seed=21, noise=0.2)
    be = hip.BackendEvaluator(w1.W, w1.H, w1.lut, w1.Wp, w1.Hp)
    be.set_fast_path()
    ref = oracle.Backend(w1.W, w1.H, w1.lut, w1.Wp, w1.Hp, 2)

    # ---- window 1 (empty map)
    be.set_window(w1.x, w1.y, w1.t_ns, 2, w1.knots_init, w1.start_ns, w1.dt_ns, w1.num_fixed, w1.t_next_win_beg_ns)
    ref.set_window(w1.x, w1.y, w1.t_ns, w1.knots_init, w1.start_ns, w1.dt_ns, w1.num_fixed, w1.t_next_win_beg_ns)
    d = np.full(w1.P, 0.002)
    c, _ = be.eval(d, False)          # "the last evaluation performed" defines IL_old (pose_graph_optimizer.cpp:303)
    c_ref, _ = ref.eval(d, False)
    assert rel_scalar(c, c_ref) < RTOL

    # visit bookkeeping first for two poses, then a second mark so some counts reach 2
    qs = [w1.knots_true[0], w1.knots_true[2], w1.knots_true[2]]
    for q in qs:
        be.setUpdateTimesIG(q, 3)
        ref.mark_visited(q, 3)
    be.updateIG(1)                    # max_update_times = 1: pixels visited twice stop accumulating
    ref.update_ig(1)
    IG, visits = be.getIG(with_visits=True)
    np.testing.assert_array_equal(visits, ref.update_times)
    assert visits.max() == 3 and (visits == 0).any()
    assert rel_img(IG, ref.IG) < RTOL
    assert 0 < IG.sum() < ref.IL_old.sum()   # some pixels were frozen by the visit count

    # ---- window 2 against the resident map
    be.set_window(w2.x, w2.y, w2.t_ns, 2, w2.knots_init, w2.start_ns, w2.dt_ns, w2.num_fixed, w2.t_next_win_beg_ns,
                  IG="resident")
    IGh = ref.IG.copy()
    ref.set_window(w2.x, w2.y, w2.t_ns, w2.knots_init, w2.start_ns, w2.dt_ns, w2.num_fixed, w2.t_next_win_beg_ns, IGh)
    for d in (np.zeros(w2.P), np.full(w2.P, -0.003)):
        c, g = be.eval(d)
        c_ref, g_ref = ref.eval(d)
        assert rel_scalar(c, c_ref) < RTOL and rel_vec(g, g_ref) < RTOL
    assert ref.alpha > 0 and rel_scalar(be.alpha, ref.alpha) < RTOL

    be.resetIG()
    IG, visits = be.getIG(with_visits=True)
    assert IG.max() == 0 and visits.max() == 0


def test_set_and_get_map_roundtrip(hip):
    w = synth.backend_window(2_000, 240, 180, 200.0, 200.0, 119.5, 89.5, 256, 128, 2, 5, 1, 0.2, seed=3)
    be = hip.reference_shaped.BackendEvaluator(w.W, w.H, w.lut, w.Wp, w.Hp)
    rng = np.random.default_rng(0)
    IG = rng.random((w.Hp, w.Wp)).astype(np.float32)
    v = rng.integers(0, 255, (w.Hp, w.Wp)).astype(np.uint8)
    be.setIG(IG, v)
    a, b = be.getIG(with_visits=True)
    np.testing.assert_array_equal(a, IG)
    np.testing.assert_array_equal(b, v)
    with pytest.raises(hip.CmaxHipError):
        be.updateIG(3)  # no evaluation has run: IL_old undefined


# ======================================================================================================================
# The upkeep kernels (mark_mask_kernel, add_mask_kernel, update_map_kernel) and the hand-over of the resident map, on the cases of
# tests/map_cases.py: the seam, the poles, the borders, saturation, both grid strides.  tests/test_map_cases_cpu.py shows that no
# case is an empty comparison and that every pose keeps every projected coordinate >= 1e-9 px from an integer, so that the device
# and the oracle truncate to the same cell: visit counts are compared EXACTLY, and so is everything that is one add per pixel.

def _dims(geom):
    g = mc.GEOMS[geom]
    return g["W"], g["H"], g["Wp"], g["Hp"]


def _evaluator(hip, geom, cls=None):
    W, H, Wp, Hp = _dims(geom)
    return (cls or hip.BackendEvaluator)(W, H, mc.lut(geom), Wp, Hp)


def _oracle(oracle, geom):
    W, H, Wp, Hp = _dims(geom)
    return oracle.Backend(W, H, mc.lut(geom), Wp, Hp, 2)


def _visits(be):
    return be.getIG(with_visits=True)[1]


def _set_window(ev, w, IG=None):
    """the same window for the device evaluator and the oracle (their set_window differ in the `order` argument only)"""
    if hasattr(ev, "updateIG"):
        ev.set_window(w.x, w.y, w.t_ns, 2, w.knots_init, w.start_ns, w.dt_ns, w.num_fixed, w.t_next_win_beg_ns, IG=IG)
    else:
        ev.set_window(w.x, w.y, w.t_ns, w.knots_init, w.start_ns, w.dt_ns, w.num_fixed, w.t_next_win_beg_ns, IG)


# ---- the footprint, exact
@pytest.mark.parametrize("geom,pose", mc.FOOTPRINTS)
def test_footprint_is_the_oracles_cell_for_cell(hip, oracle, geom, pose):
    second = mc.second_pose(geom, pose)
    for r in mc.GEOM_RADII[geom]:
        be, ref = _evaluator(hip, geom), _oracle(oracle, geom)      # fresh: counts and scratch mask as the library creates them
        be.setUpdateTimesIG(mc.quat(pose), r)
        ref.mark_visited(mc.quat(pose), r)
        v = _visits(be)
        print("%s/%s r=%d: %d cells marked, %d differ from the oracle" % (geom, pose, r, int(v.sum()), int((v != ref.update_times).sum())))
        np.testing.assert_array_equal(v, ref.update_times)
        assert v.max() == 1 and v.any()
        # a second, different pose: a scratch mask that was not cleared would add the first footprint once more
        be.setUpdateTimesIG(mc.quat(second), r)
        ref.mark_visited(mc.quat(second), r)
        np.testing.assert_array_equal(_visits(be), ref.update_times)
        assert ref.update_times.max() <= 2
        be.close()


@pytest.mark.parametrize("geom,pose", [("p130", "seam"), ("p2048", "mid")])
def test_reset_between_two_marks(hip, oracle, geom, pose):
    be, ref = _evaluator(hip, geom), _oracle(oracle, geom)
    be.setUpdateTimesIG(mc.quat(pose), 3)
    be.resetIG()
    IG, v = be.getIG(with_visits=True)
    assert not v.any() and not IG.any()
    second = mc.second_pose(geom, pose)
    be.setUpdateTimesIG(mc.quat(second), 3)
    ref.mark_visited(mc.quat(second), 3)          # the oracle never saw the first pose
    np.testing.assert_array_equal(_visits(be), ref.update_times)
    assert ref.update_times.max() == 1


# ---- saturation
def test_counts_saturate_at_255(hip):
    geom, poses, r = "p512", ("seam", "seam", "seam_neg"), 3
    _, _, Wp, Hp = _dims(geom)
    start = np.tile(np.array([0, 1, 253, 254, 255], np.uint8)[np.arange(Wp) % 5], (Hp, 1))   # stripes across the footprints
    hits = sum(mc.mask(geom, p, r).astype(np.int32) for p in poses)
    for v0 in (0, 1, 253, 254, 255):
        assert {int(h) for h in np.unique(hits[start == v0])} == {0, 1, 2, 3}     # every start value meets every hit count
    be = _evaluator(hip, geom)
    be.setIG(visits=start)
    for p in poses:
        be.setUpdateTimesIG(mc.quat(p), r)
    v = _visits(be)
    want = np.minimum(start.astype(np.int32) + hits, 255).astype(np.uint8)
    print("saturation: %d cells at 255 afterwards (%d before), %d differ" % (int((v == 255).sum()), int((start == 255).sum()),
                                                                            int((v != want).sum())))
    np.testing.assert_array_equal(v, want)
    np.testing.assert_array_equal(v[hits == 0], start[hits == 0])                 # outside the footprints: untouched
    assert (want[start == 253] == 255).any() and (want[start == 253] == 254).any() and not (want < start).any()


# ---- the update gate, bitwise
@pytest.mark.parametrize("geom", ["p130", "p2048"])
def test_update_gate_is_bitwise_where_the_count_allows(hip, geom):
    _, _, Wp, Hp = _dims(geom)
    npix = Wp * Hp
    w = mc.window(geom, "mid")
    be = _evaluator(hip, geom)
    _set_window(be, w)
    be.eval(np.full(w.P, 0.002), False)
    IL = be.get_plane(_lib.PLANE_IL_OLD)
    voted = IL != 0
    assert voted.sum() > 50
    if npix > mc.UPDATE_LANES:
        assert voted.reshape(-1)[mc.UPDATE_LANES:].any()          # votes past the first step of the update kernel's grid
    rng = np.random.default_rng(5)
    IG0 = rng.random((Hp, Wp)).astype(np.float32) * np.float32(3.0)
    visits = rng.permutation(np.arange(npix) % 256).astype(np.uint8).reshape(Hp, Wp)
    near = {0, 1, 2, 254, 255}
    filler = iter(rng.permutation(np.flatnonzero(voted.reshape(-1))))
    for val in sorted(near):                                      # every value next to a threshold sits on a pixel with votes
        visits.reshape(-1)[next(filler)] = val
    assert set(np.unique(visits)) == set(range(256)) and near <= set(np.unique(visits[voted]))
    for m in (-1, 0, 1, 254, 255):
        be.setIG(IG0, visits)
        be.updateIG(m)
        IG, v = be.getIG(with_visits=True)
        want = np.where(visits.astype(np.int32) <= m, IG0 + IL, IG0).astype(np.float32)      # one fp32 add per pixel: no order to vary
        diff = int((IG.view(np.uint32) != want.view(np.uint32)).sum())
        print("%s updateIG(%d): %d pixels updated, %d differ bitwise" % (geom, m, int(((visits.astype(np.int32) <= m) & voted).sum()), diff))
        assert diff == 0
        np.testing.assert_array_equal(v, visits)
        assert (m < 0) == (not ((visits.astype(np.int32) <= m) & voted).any())
        assert ((visits.astype(np.int32) > m) & voted).any() == (m < 255)


# ---- what "the last evaluation" is
def _arrive(be, how, P):
    """run evaluations on `be` that end at x (or wherever a solve ends); returns the last point, or None if only the evaluator
    knows it"""
    x = 0.004 * np.sin(np.arange(P) + 1.0)
    far, mid = np.full(P, 0.25), np.full(P, -0.1)   # 14 degrees off: their votes lie elsewhere, stale planes would show in the sum
    be.eval(far, True)                         # whatever came before the last evaluation: both ping-pong buffers have been used
    be.eval(mid, False)
    if how == "eval_grad":
        be.eval(x, True)
    elif how == "eval_cost":
        be.eval(x, False)
    elif how == "repeat":                      # the second call finds the image of the first resident
        be.eval(x, False)
        be.eval(x, True)
    elif how == "accumulate_finish":
        be.accumulate(x, True)
        be.finish(True)
    elif how == "eval_many":
        be.eval_many(np.stack([far, mid, x]), True)
    elif how == "eval_each":
        be.eval_each(np.stack([far, mid, x]), False)
    elif how == "prepare_eval":
        be.prepare(far)
        be.eval(x, True)
    elif how == "eval_prepare":                # a prepare queues no evaluation: the last one is still the eval before it
        be.eval(x, True)
        be.prepare(far)
    elif how == "solve":
        be.setupProblemAndOptimize(x)
        return None
    else:
        raise AssertionError(how)
    return x


@pytest.mark.parametrize("how", ["eval_grad", "eval_cost", "repeat", "accumulate_finish", "eval_many", "eval_each", "prepare_eval",
                                 "eval_prepare", "solve"])
@pytest.mark.parametrize("mode", ["default", "fast", "reference_shaped", "deterministic"])
def test_update_folds_in_the_last_evaluation(hip, oracle, mode, how):
    geom = "p512"
    w = mc.window(geom, "seam")
    be = _evaluator(hip, geom, hip.reference_shaped.BackendEvaluator if mode == "reference_shaped" else None)
    if mode == "fast":
        be.set_fast_path()
    if mode == "deterministic":
        be.set_deterministic()
    _set_window(be, w)
    x = _arrive(be, how, w.P)
    IL = be.get_plane(_lib.PLANE_IL_OLD)
    be.updateIG(255)
    IG, v = be.getIG(with_visits=True)
    assert not v.any()
    assert IG.tobytes() == IL.tobytes()                      # empty map + IL_old, one add per pixel

    if x is not None:       # the oracle at the same point
        ref = _oracle(oracle, geom)
        _set_window(ref, w)
        ref.eval(x, False)
        want = ref.IL_old
        knots = oracle.left_update(w.knots_init, x, w.num_fixed)
        rot = lambda t: oracle.spline_eval(2, knots, w.start_ns, w.dt_ns, t, jac=False)[1]
    else:                   # a solve ends where it ends: the point is the evaluator's pose table at its last evaluation
        R, _, _, tb = be.get_pose_table()
        table = {int(t): r for t, r in zip(tb, R)}
        rot = lambda t: table[int(t)]
        want, _, _ = iwe_numpy.backend_iwe(w.x, w.y, w.t_ns, mc.lut(geom), w.W, w.Wp, w.Hp, 2, w.num_fixed, w.t_next_win_beg_ns,
                                           w.batch, w.sample_rate, lambda t: (rot(t), None, 0), want_deriv=False)
    n = mc.old_votes_inside(w, mc.lut(geom), rot)
    s = float(IL.sum(dtype=np.float64))
    print("%s after %s: IL_old vs oracle %.2e, sum %.6f for %d votes (%.2e)" % (mode, how, rel_img(IL, want), s, n, abs(s - n) / n))
    assert n > 1000
    assert rel_img(IL, want) < RTOL
    assert abs(s - n) < RTOL * n                             # stale or skipped tiles would add or lose whole votes

    _set_window(be, w)                                       # a new window: its IL_old does not exist yet
    with pytest.raises(hip.CmaxHipError):
        be.updateIG(255)
    assert be.getIG().tobytes() == np.zeros_like(IG).tobytes()


# ---- the resident map into the next window
def _second_window_matches(be, ref, w2, expect_alpha):
    for d in (np.zeros(w2.P), np.full(w2.P, -0.003)):
        c, g = be.eval(d)
        c_ref, g_ref = ref.eval(d)
        print("  contrast %.3e, gradient %.3e, alpha %.9g vs %.9g" % (rel_scalar(c, c_ref), rel_vec(g, g_ref), be.alpha, ref.alpha))
        assert rel_scalar(c, c_ref) < RTOL and rel_vec(g, g_ref) < RTOL
    if expect_alpha:
        assert ref.alpha > 0 and rel_scalar(be.alpha, ref.alpha) < RTOL
    else:
        assert ref.alpha == 0.0 and be.alpha == 0.0


@pytest.mark.parametrize("pose", ["seam", "north"])
def test_resident_map_at_the_seam_and_at_the_pole(hip, oracle, pose):
    geom = "p512"
    w1, w2 = mc.window(geom, pose, num_fixed=1), mc.window(geom, pose, num_fixed=0, noise=0.2)
    be, ref = _evaluator(hip, geom), _oracle(oracle, geom)
    _set_window(be, w1)
    _set_window(ref, w1)
    d = np.full(w1.P, 0.002)
    be.eval(d, False)
    ref.eval(d, False)
    partner = mc.PARTNERS[pose][0]                           # overlaps the footprint in part: where it does the map stays empty
    for name in (pose, pose, partner):
        be.setUpdateTimesIG(mc.quat(name), 3)
        ref.mark_visited(mc.quat(name), 3)
    be.updateIG(2)
    ref.update_ig(2)
    IG, v = be.getIG(with_visits=True)
    np.testing.assert_array_equal(v, ref.update_times)
    assert rel_img(IG, ref.IG) < RTOL
    frozen = (ref.update_times > 2) & (ref.IL_old != 0)
    print("%s: %d pixels of the map hold votes, %d with votes stay empty" % (pose, int((IG != 0).sum()), int(frozen.sum())))
    assert frozen.sum() > 50 and not IG[frozen].any() and (IG != 0).sum() > 50
    if pose == "seam":
        assert IG[:, :8].any() and IG[:, -8:].any()          # the map lies on both sides of the seam
    else:
        assert IG[:8].any()
    _set_window(be, w2, IG="resident")
    _set_window(ref, w2, IG=ref.IG.copy())
    _second_window_matches(be, ref, w2, expect_alpha=True)


@pytest.mark.parametrize("nonzero", [0, 1])
def test_resident_map_that_is_empty_or_one_pixel(hip, oracle, nonzero):
    """the host does not know what a resident map holds: the device's own non-zero count decides alpha"""
    geom = "p512"
    _, _, Wp, Hp = _dims(geom)
    w2 = mc.window(geom, "mid", num_fixed=0, noise=0.2)
    be, ref = _evaluator(hip, geom), _oracle(oracle, geom)
    IG = np.zeros((Hp, Wp), np.float32)
    if nonzero:
        ref0 = _oracle(oracle, geom)
        _set_window(ref0, w2)
        ref0.eval(np.zeros(w2.P), False)
        y, x = np.unravel_index(np.argmax(ref0.IL_old + ref0.IL_new), IG.shape)     # a pixel inside the window's own image
        IG[y, x] = 2.5
    be.setIG(IG, np.zeros((Hp, Wp), np.uint8))
    _set_window(be, w2, IG="resident")
    _set_window(ref, w2, IG=IG)
    _second_window_matches(be, ref, w2, expect_alpha=bool(nonzero))
    np.testing.assert_array_equal(be.getIG(), IG)            # the window read the map, nothing wrote it


# ---- four windows, one resident map
def test_four_windows_across_the_seam(hip, oracle):
    geom, poses = mc.SEQUENCE
    be, ref = _evaluator(hip, geom), _oracle(oracle, geom)
    for k, pose in enumerate(poses):
        w = mc.window(geom, pose, seed=21 + k)
        _set_window(be, w, IG="resident" if k else None)
        _set_window(ref, w, IG=ref.IG.copy() if k else None)
        d = np.full(w.P, 0.002)
        c, _ = be.eval(d, False)
        c_ref, _ = ref.eval(d, False)
        assert rel_scalar(c, c_ref) < RTOL
        assert (ref.alpha > 0) == (k > 0) and rel_scalar(be.alpha, ref.alpha) < RTOL
        before, seen = be.getIG(with_visits=True)            # the device's own map as this window found it
        IL = be.get_plane(_lib.PLANE_IL_OLD)
        be.updateIG(1)
        ref.update_ig(1)
        for q in (w.knots_true[0], w.knots_true[2]):
            be.setUpdateTimesIG(q, 3)
            ref.mark_visited(q, 3)
        IG, v = be.getIG(with_visits=True)
        print("window %d (%s): alpha %.6g, IG vs oracle %.2e, counts up to %d, %d differ"
              % (k, pose, ref.alpha, rel_img(IG, ref.IG), int(v.max()), int((v != ref.update_times).sum())))
        np.testing.assert_array_equal(v, ref.update_times)
        assert rel_img(IG, ref.IG) < RTOL
    voted = IL != 0
    frozen, open_ = voted & (seen > 1), voted & (seen <= 1)
    assert frozen.any() and open_.any()                      # the last window met pixels of both kinds ...
    np.testing.assert_array_equal(IG[frozen], before[frozen])   # ... these kept their value
    np.testing.assert_array_equal(IG[open_], (before + IL)[open_])   # ... and these took its votes
    assert (IG[open_] > before[open_]).any() and before[frozen].any()
    assert (v > 1).any() and (v <= 1).any()


# ---- status codes
def test_upkeep_status_codes(hip):
    geom = "p64"
    be = _evaluator(hip, geom)
    be.setUpdateTimesIG(mc.quat("mid"), 1)
    counts = _visits(be)
    assert counts.any()
    L = _lib.lib()
    q = np.ascontiguousarray(mc.quat("left"))
    qp = q.ctypes.data_as(_lib.C.POINTER(_lib.C.c_double))
    assert L.cmx_backend_mark_visited(be._ctx, qp, -1) == _lib.ERR_INVALID_ARG
    assert L.cmx_backend_mark_visited(be._ctx, qp, 65) == _lib.ERR_INVALID_ARG
    assert L.cmx_backend_mark_visited(be._ctx, None, 3) == _lib.ERR_INVALID_ARG
    assert L.cmx_backend_update_map(be._ctx, 1) == _lib.ERR_STATE            # no evaluation yet
    with pytest.raises(hip.CmaxHipError):
        be.setUpdateTimesIG(mc.quat("left"), 65)
    p = synth.frontend_packet(2_000, 240, 180, 200.0, 200.0, 119.5, 89.5, seed=3)
    fe = hip.FrontendEvaluator(p.W, p.H, p.lut)
    assert L.cmx_backend_mark_visited(fe._ctx, qp, 3) == _lib.ERR_STATE
    assert L.cmx_backend_update_map(fe._ctx, 1) == _lib.ERR_STATE
    assert L.cmx_backend_reset_map(fe._ctx) == _lib.ERR_STATE
    np.testing.assert_array_equal(_visits(be), counts)                       # none of them touched the counts
    assert L.cmx_backend_mark_visited(be._ctx, qp, 64) == _lib.OK            # the largest radius is accepted
    assert _visits(be).sum() > counts.sum()
