"""GPU: whole-trajectory panorama reconstruction (cmx_backend_recon_* / BackendEvaluator.reconstruct_*) against the CPU oracle's
vote loop, for splines longer than a bundle-adjustment window can be (K = 100 cubic, K = 70 linear, K = 2^20), every shape at
which the fused pose + vote kernel takes another path, the three ingest paths, deterministic mode, the product's own window
path, isolation from the evaluation state, the tone map and the error codes.  Configurations and oracle planes: recon_cases.py
(tests/test_recon_inputs_cpu.py shows on the CPU that none of them compares two empty planes)."""
import numpy as np
import pytest

import recon_cases as rc
from cmax_slam_amd import _lib, synth
from util import RTOL, rel_img

pytestmark = pytest.mark.gpu
W, H = rc.SENSOR[:2]


def make(hip, name, deterministic=False):
    c, w = rc.CASES[name], rc.window(name)[0]
    be = hip.BackendEvaluator(W, H, w.lut, c["Wp"], c["Hp"])
    if deterministic:
        be.set_deterministic(True)
    return be


def begin(be, name):
    c, w = rc.CASES[name], rc.window(name)[0]
    be.reconstruct_begin(c["order"], w.knots_true, w.start_ns, w.dt_ns, c["batch"], c["rate"])


def run(be, name, pieces=None, how="add"):
    """begin, one add per piece (default: the whole stream), get with counters, end"""
    _, x, y, t = rc.window(name)
    begin(be, name)
    for lo, hi in (pieces or [(0, len(x))]):
        if how == "add":
            be.reconstruct_add(x[lo:hi], y[lo:hi], t[lo:hi])
        else:
            be.reconstruct_add_aos(_lib.dvs_events(x[lo:hi], y[lo:hi], t[lo:hi]))
    out = be.reconstruct_get(with_counts=True)
    be.reconstruct_end()
    return out


def check_counts(name, plane, n_sampled, n_inside, pieces=None):
    c = rc.CASES[name]
    want = sum(rc.sampled(hi - lo, c["batch"], c["rate"]) for lo, hi in (pieces or [(0, c["N"])]))
    assert n_sampled == want
    assert 0 <= n_inside <= n_sampled
    assert abs(n_inside - float(plane.sum(dtype=np.float64))) <= 1e-5 * max(n_inside, 1) * (n_inside > 0)


def test_long_cubic_spline(hip, oracle):
    """A: order 4, K = 100 -- cmx_backend_set_window refuses this spline; one add of 60 007 events"""
    be = make(hip, "A")
    plane, n_sampled, n_inside = run(be, "A")
    ref = rc.oracle_plane(oracle, "A")
    r = rel_img(plane, ref)
    print("A: rel_img %.2e, sampled %d, inside %d, votes %.3f" % (r, n_sampled, n_inside, plane.sum(dtype=np.float64)))
    assert r < RTOL
    assert n_sampled == 60_007
    assert abs(n_inside - float(plane.sum(dtype=np.float64))) < 1e-5 * n_inside
    check_counts("A", plane, n_sampled, n_inside)


def test_linear_sliced_subsampled(hip, oracle):
    """B: order 2, K = 70, batch 64, rate 3.  Slices at batch multiples add up to the whole stream's loop; a cut that is not a
    batch multiple makes every call its own loop (its last, single event is skipped)."""
    be = make(hip, "B")
    pieces = rc.cuts("B", 7 * 64, 100 * 64)
    plane, n_sampled, n_inside = run(be, "B", pieces)
    r = rel_img(plane, rc.oracle_plane(oracle, "B"))
    print("B, cuts at batch multiples: rel_img %.2e, sampled %d" % (r, n_sampled))
    assert r < RTOL
    assert n_sampled == 10_313 == rc.sampled(30_001, 64, 3)
    check_counts("B", plane, n_sampled, n_inside, pieces)

    _, x, y, t = rc.window("B")
    pieces = rc.cuts("B", 7 * 64, 7 * 64 + 5 * 64 + 1)
    plane, n_sampled, n_inside = run(be, "B", pieces)
    ref = np.zeros(plane.shape, np.float64)
    for lo, hi in pieces:
        ref += rc.oracle_loop(oracle, "B", x[lo:hi], y[lo:hi], t[lo:hi])
    r = rel_img(plane, ref)
    print("B, one slice of 5 * 64 + 1 events: rel_img %.2e, sampled %d" % (r, n_sampled))
    assert r < RTOL
    check_counts("B", plane, n_sampled, n_inside, pieces)
    assert n_sampled != 10_313  # (the skipped single event and the restarted batches change the sampling)


@pytest.mark.parametrize("name", ["batch1", "batch3", "batch5000", "n0", "n1", "n2", "n65", "pano130x96", "pano1000x300", "poles",
                                  "shortest4", "shortest2"])
def test_edge_shapes(hip, oracle, name):
    be = make(hip, name)
    plane, n_sampled, n_inside = run(be, name)
    ref = rc.oracle_plane(oracle, name)
    r = rel_img(plane, ref)
    print("%s: rel_img %.2e, sampled %d, inside %d" % (name, r, n_sampled, n_inside))
    assert plane.shape == ref.shape
    assert r < RTOL
    check_counts(name, plane, n_sampled, n_inside)
    if name == "poles":
        assert n_inside < n_sampled  # votes at the seam / the poles are dropped by the border rule
    elif rc.CASES[name]["N"] >= 2:
        assert n_inside == n_sampled


def test_a_million_knots(hip, oracle):
    """K = 2^20 (32 MB of knots on the device): B's spline at the far end of a long identity trajectory"""
    c, (w, x, y, t) = rc.CASES["B"], rc.window("B")
    K = 1 << 20
    off = K - c["K"]
    knots = np.zeros((K, 4))
    knots[:, 3] = 1.0
    knots[off:] = w.knots_true
    be = make(hip, "B")
    be.reconstruct_begin(2, knots, w.start_ns - off * w.dt_ns, w.dt_ns, c["batch"], c["rate"])
    be.reconstruct_add(x, y, t)
    plane = be.reconstruct_get()
    be.reconstruct_end()
    assert rel_img(plane, rc.oracle_plane(oracle, "B")) < RTOL


def _three_paths(hip, name, deterministic):
    _, x, y, t = rc.window(name)
    be = make(hip, name, deterministic)
    a = run(be, name)
    b = run(be, name, how="aos")
    store = hip.EventStore(W, H, len(x))
    store.push(x, y, t)
    begin(be, name)
    be.reconstruct_add_from(store, 0, len(x))
    c = be.reconstruct_get(with_counts=True)
    # a sub-range of the store against the same events from the host
    lo, hi = 7 * 64, 7 * 64 + 5 * 64 + 1
    begin(be, name)
    be.reconstruct_add_from(store, lo, hi - lo)
    sub_store = be.reconstruct_get()
    begin(be, name)
    be.reconstruct_add(x[lo:hi], y[lo:hi], t[lo:hi])
    sub_host = be.reconstruct_get()
    be.reconstruct_end()
    store.close()
    return a, b, c, sub_store, sub_host


def test_ingest_paths_deterministic_bit_identical(hip, oracle):
    a, b, c, sub_store, sub_host = _three_paths(hip, "B", True)
    assert a[1:] == b[1:] == c[1:]
    np.testing.assert_array_equal(a[0], b[0])
    np.testing.assert_array_equal(a[0], c[0])
    np.testing.assert_array_equal(sub_store, sub_host)
    assert sub_host.sum() > 50
    assert rel_img(a[0], rc.oracle_plane(oracle, "B")) < RTOL


def test_ingest_paths_default_mode_agree(hip, oracle):
    a, b, c, sub_store, sub_host = _three_paths(hip, "B", False)
    ref = rc.oracle_plane(oracle, "B")
    assert a[1:] == b[1:] == c[1:]
    for p in (a[0], b[0], c[0]):
        assert rel_img(p, ref) < RTOL
    assert rel_img(sub_store, sub_host) < RTOL


def test_deterministic(hip, oracle):
    be = make(hip, "A", deterministic=True)
    p1 = run(be, "A")
    p2 = run(be, "A")
    p3 = run(be, "A", rc.cuts("A", 70 * 100, 400 * 100))
    np.testing.assert_array_equal(p1[0], p2[0])
    np.testing.assert_array_equal(p1[0], p3[0])
    assert p1[1:] == p2[1:] == p3[1:]
    assert rel_img(p1[0], rc.oracle_plane(oracle, "A")) < RTOL
    # the mode is the one recorded at begin: switching the option in the middle changes nothing
    begin(be, "A")
    be.set_deterministic(False)
    _, x, y, t = rc.window("A")
    be.reconstruct_add(x, y, t)
    np.testing.assert_array_equal(be.reconstruct_get(), p1[0])
    be.reconstruct_end()


def test_internal_slices(hip, oracle):
    """cmx_diag_set(CMX_DIAG_RECON_SLICE_EVENTS): the same call cut into many internal slices -- double-buffered staging on the
    host paths, one slice-sized batch-time table on the store path -- is bitwise the one-slice result in deterministic mode"""
    L = _lib.lib()
    _, x, y, t = rc.window("B")
    whole = _three_paths(hip, "B", True)
    try:
        for n_slice in (1000, 64):  # 15 batches per slice (the last slice is partial), one batch per slice
            assert L.cmx_diag_set(_lib.DIAG_RECON_SLICE_EVENTS, n_slice) == 0
            sliced = _three_paths(hip, "B", True)
            for p, q in zip(whole, sliced):
                np.testing.assert_array_equal(p[0] if isinstance(p, tuple) else p, q[0] if isinstance(q, tuple) else q)
            assert whole[0][1:] == sliced[0][1:] == sliced[1][1:] == sliced[2][1:]
        assert L.cmx_diag_set(_lib.DIAG_RECON_SLICE_EVENTS, 1000) == 0
        be = make(hip, "A")
        plane, n_sampled, n_inside = run(be, "A")  # default mode, cubic, 61 slices
        assert rel_img(plane, rc.oracle_plane(oracle, "A")) < RTOL
        check_counts("A", plane, n_sampled, n_inside)
    finally:
        assert L.cmx_diag_set(_lib.DIAG_RECON_SLICE_EVENTS, 0) == 0
    assert L.cmx_diag_set(_lib.DIAG_RECON_SLICE_EVENTS, -1) != 0


def test_against_the_window_path(hip):
    """K = 10 cubic, sigma = 0: IL_old + IL_new of a cost-only evaluation at zero increments is the same vote loop"""
    c, (w, x, y, t) = rc.CASES["window"], rc.window("window")
    be = make(hip, "window")
    be.set_window(x, y, t, c["order"], w.knots_true, w.start_ns, w.dt_ns, 0, w.t_next_win_beg_ns, c["batch"], c["rate"],
                  blur_sigma=0.0)
    be.eval(np.zeros(be.num_params), want_grad=False)
    old, new = be.get_plane(_lib.PLANE_IL_OLD), be.get_plane(_lib.PLANE_IL_NEW)
    assert old.sum() > 1000 and new.sum() > 1000
    plane = be.reconstruct(x, y, t, c["order"], w.knots_true, w.start_ns, w.dt_ns, event_batch_size=c["batch"],
                           event_sample_rate=c["rate"])
    assert rel_img(plane, old.astype(np.float64) + new) < RTOL


def test_evaluation_state_untouched(hip):
    c, (w, x, y, t) = rc.CASES["window"], rc.window("window")
    be = make(hip, "window", deterministic=True)
    be.set_window(x, y, t, c["order"], w.knots_init, w.start_ns, w.dt_ns, 2, w.t_next_win_beg_ns, c["batch"], c["rate"])
    rng = np.random.default_rng(3)
    xa, xb = rng.normal(0, 0.01, be.num_params), rng.normal(0, 0.01, be.num_params)
    be.eval(xa)
    be.updateIG(200)
    be.setUpdateTimesIG(w.knots_true[3], 3)

    def reads():
        ca, ga = be.eval(xa)
        cb, gb = be.eval(xb)
        ig, visits = be.getIG(with_visits=True)
        return (np.float64(ca).tobytes(), ga.tobytes(), np.float64(cb).tobytes(), gb.tobytes(), ig.tobytes(), visits.tobytes(),
                be.get_plane(_lib.PLANE_IL_OLD).tobytes(), np.float64(be.alpha).tobytes())
    reads()
    before = reads()
    begin(be, "window")
    be.reconstruct_add(x, y, t)
    plane, n_sampled, n_inside = be.reconstruct_get(with_counts=True)
    be.reconstruct_render(0.75)
    be.reconstruct_render(1.0, w.knots_true[5])
    be.reconstruct_end()
    assert n_inside == n_sampled == c["N"] and plane.sum() > 0.99 * c["N"]
    after = reads()
    assert before == after


def test_render_is_the_map_tone_map(hip):
    c, (w, x, y, t) = rc.CASES["window"], rc.window("window")
    be, other = make(hip, "window"), make(hip, "window")
    begin(be, "window")
    blank = be.reconstruct_render(0.75)
    assert blank.shape == (c["Hp"], c["Wp"]) and (blank == 255).all()
    assert (be.reconstruct_render(1.0, w.knots_true[0])[..., 1] == 255).sum() >= c["Hp"] * c["Wp"] - 2 * (W + H)
    be.reconstruct_add(x, y, t)
    other.setIG(be.reconstruct_get())
    for gamma in (1.0, 0.75):
        mono = be.reconstruct_render(gamma)
        assert mono.dtype == np.uint8 and mono.min() == 0 and mono.max() == 255
        np.testing.assert_array_equal(mono, other.publishEventImage(gamma))
        bgr = be.reconstruct_render(gamma, w.knots_true[4])
        assert bgr.shape == (c["Hp"], c["Wp"], 3)
        np.testing.assert_array_equal(bgr, other.publishEventImage(gamma, w.knots_true[4]))
    with pytest.raises(hip.CmaxHipError) as e:
        be.reconstruct_render(0.0)
    assert e.value.status == _lib.ERR_INVALID_ARG
    be.reconstruct_end()


def _status(hip, fn, *a, **k):
    with pytest.raises(hip.CmaxHipError) as e:
        fn(*a, **k)
    return e.value.status


def test_state_and_argument_errors(hip):
    c, (w, x, y, t) = rc.CASES["window"], rc.window("window")
    be = make(hip, "window")
    assert _status(hip, be.reconstruct_add, x, y, t) == _lib.ERR_STATE
    assert _status(hip, be.reconstruct_add_aos, _lib.dvs_events(x, y, t)) == _lib.ERR_STATE
    assert _status(hip, be.reconstruct_get) == _lib.ERR_STATE
    assert _status(hip, be.reconstruct_render) == _lib.ERR_STATE
    store = hip.EventStore(W, H, 16)
    assert _status(hip, be.reconstruct_add_from, store, 0, 0) == _lib.ERR_STATE
    store.close()
    be.reconstruct_end()  # nothing to free: not an error
    k, s, d = w.knots_true, w.start_ns, w.dt_ns
    assert _status(hip, be.reconstruct_begin, 3, k, s, d) == _lib.ERR_INVALID_ARG
    assert _status(hip, be.reconstruct_begin, 4, k[:3], s, d) == _lib.ERR_INVALID_ARG
    assert _status(hip, be.reconstruct_begin, 2, k[:1], s, d) == _lib.ERR_INVALID_ARG
    assert _status(hip, be.reconstruct_begin, 4, k, s, 0) == _lib.ERR_INVALID_ARG
    assert _status(hip, be.reconstruct_begin, 4, k, s, -5) == _lib.ERR_INVALID_ARG
    assert _status(hip, be.reconstruct_begin, 4, k, s, d, event_batch_size=0) == _lib.ERR_INVALID_ARG
    assert _status(hip, be.reconstruct_begin, 4, k, s, d, event_sample_rate=0) == _lib.ERR_INVALID_ARG
    assert _status(hip, be.reconstruct_get) == _lib.ERR_STATE  # a refused begin begins nothing


def test_a_failed_add_adds_nothing(hip, oracle):
    c, (w, x, y, t) = rc.CASES["window"], rc.window("window")
    be = make(hip, "window")
    begin(be, "window")
    be.reconstruct_add(x[:5000], y[:5000], t[:5000])
    good = be.reconstruct_get(with_counts=True)
    assert good[1] == good[2] == 5000

    def unchanged():
        now = be.reconstruct_get(with_counts=True)
        np.testing.assert_array_equal(now[0], good[0])
        assert now[1:] == good[1:]

    # an event outside the sensor, near the END of the input: everything is validated before the first vote
    bad_x = x.copy()
    bad_x[-2] = W
    assert _status(hip, be.reconstruct_add, bad_x, y, t) == _lib.ERR_EVENT_RANGE
    unchanged()
    bad_y = y.copy()
    bad_y[-2] = H
    assert _status(hip, be.reconstruct_add_aos, _lib.dvs_events(x, bad_y, t)) == _lib.ERR_EVENT_RANGE
    unchanged()
    # stamps shifted by 10 s leave the knot support (the oracle refuses this input with rc -2)
    late = t + 10_000_000_000
    with pytest.raises(ValueError, match="rc=-2"):
        rc.oracle_loop(oracle, "window", x, y, late)
    assert _status(hip, be.reconstruct_add, x, y, late) == _lib.ERR_SPLINE_RANGE
    unchanged()
    only_tail = t.copy()
    only_tail[-150:] += 10_000_000_000  # the last two batches alone
    assert _status(hip, be.reconstruct_add, x, y, only_tail) == _lib.ERR_SPLINE_RANGE
    unchanged()
    store = hip.EventStore(W, H, len(x))
    store.push(x, y, only_tail)
    assert _status(hip, be.reconstruct_add_from, store, 0, len(x)) == _lib.ERR_SPLINE_RANGE
    unchanged()
    assert _status(hip, be.reconstruct_add_from, store, 0, len(x) + 1) == _lib.ERR_INVALID_ARG
    unchanged()
    store.close()
    # a batch whose first event is later than its last one
    back = t.copy()
    back[19_900] = t[19_999] + 1000
    assert _status(hip, be.reconstruct_add, x, y, back) == _lib.ERR_TIME_ORDER
    unchanged()
    store = hip.EventStore(W, H, len(x))
    store.push(x, y, back)
    assert _status(hip, be.reconstruct_add_from, store, 0, len(x)) == _lib.ERR_TIME_ORDER
    unchanged()
    store.close()
    # ... and the reconstruction goes on from where it was
    be.reconstruct_add(x[5000:], y[5000:], t[5000:])
    plane = be.reconstruct_get()
    be.reconstruct_end()
    assert rel_img(plane, rc.oracle_plane(oracle, "window")) < RTOL


def test_group_handle_has_no_reconstruction(hip):
    c, (w, x, y, t) = rc.CASES["window"], rc.window("window")
    grp = hip.BackendEvaluator(W, H, w.lut, c["Wp"], c["Hp"], devices=[0, 0], transport=_lib.GROUP_DIRECT)
    assert _status(hip, grp.reconstruct_begin, c["order"], w.knots_true, w.start_ns, w.dt_ns) == _lib.ERR_STATE
    assert _status(hip, grp.reconstruct_add, x, y, t) == _lib.ERR_STATE
    assert _status(hip, grp.reconstruct_get) == _lib.ERR_STATE
    assert _status(hip, grp.reconstruct_render) == _lib.ERR_STATE
    assert _status(hip, grp.reconstruct_end) == _lib.ERR_STATE
    grp.close()


def test_example_reconstructs_along_the_whole_trajectory(hip, tmp_path):
    import os
    import sys
    ex = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples")
    if ex not in sys.path:
        sys.path.insert(0, ex)
    import rotation_pipeline as rp
    stream = synth.event_stream(2e6, 0.5, 240, 180, 200.0, 200.0, 119.5, 89.5, omega_mean=(0.2, 1.8, 0.3),
                                omega_amp=(1.0, 0.8, 1.0), seed=77)
    res = rp.run_pipeline(stream, rp.Params(), reconstruct=True, display_prefix=str(tmp_path / "shot"))
    traj = res["traj"]
    t_hi = traj.t_beg_ns + (traj.size() - traj.order + 1) * traj.dt_ns
    n_in = int(np.searchsorted(stream.t_ns, t_hi) - np.searchsorted(stream.t_ns, traj.t_beg_ns))
    assert res["recon"].shape == res["IG"].shape and res["recon"].dtype == np.float32
    assert n_in > 0.5 * len(stream.t_ns)
    assert float(res["recon"].sum(dtype=np.float64)) >= 0.5 * len(stream.t_ns)
    assert float(res["recon"].sum(dtype=np.float64)) <= n_in * (1 + 1e-5)
    Hp, Wp = res["IG"].shape
    pgm = (tmp_path / "shot_recon.pgm").read_bytes()
    head = b"P5\n%d %d\n255\n" % (Wp, Hp)
    assert pgm.startswith(head) and len(pgm) == len(head) + Wp * Hp
    img = np.frombuffer(pgm[len(head):], np.uint8)
    assert img.max() == 255 and img.min() == 0
    # the default path does not reconstruct
    short = synth.event_stream(2e6, 0.3, 240, 180, 200.0, 200.0, 119.5, 89.5, omega_mean=(0.2, 1.8, 0.3),
                               omega_amp=(1.0, 0.8, 1.0), seed=78)
    plain = rp.run_pipeline(short, rp.Params())
    assert "recon" not in plain
