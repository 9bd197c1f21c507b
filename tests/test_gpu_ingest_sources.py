"""-m gpu: the same events through every source a consumer accepts -- host arrays, the host's own records, a cut from an
EventStore -- for the three consumers (front-end packet, back-end window, reconstruction add) and the group form of the window.
Whatever the source, the device holds the same words: deterministic evaluators must agree bit for bit, every bad input must give
the same status, and a failed hand-over must leave nothing behind.  Window sizes sit on the edges of the batch rule (B = 64): the
one-event window, a trailing single event that no batch holds, a short last batch."""
import functools

import numpy as np
import pytest

import recon_cases
from cmax_slam_amd import _lib, dist, synth
from util import RTOL, rel_img, rel_scalar, rel_vec

pytestmark = pytest.mark.gpu

W, H, WP, HP, B = 240, 180, 512, 256, 64
CAM = (W, H, 200.0, 200.0, 119.5, 89.5)
SIZES = [1, 2, 65, 129, 130, 4_099]
RATES = [1, 3]
OFF = 37            # the cut starts here: the store holds a prefix the window does not
N_GEN = OFF + 4_099
OMEGAS = [(0.0, 0.0, 0.0), (0.6, -0.9, 0.4)]


@functools.lru_cache(maxsize=None)
def packet():
    return synth.frontend_packet(N_GEN, *CAM, seed=71)


@functools.lru_cache(maxsize=None)
def window():
    return synth.backend_window(N_GEN, *CAM, WP, HP, 4, 10, 2, 0.30, seed=72)


def cut(s, n, t=None):
    """events [OFF, OFF + n) of a synthetic stream (t: its timestamps replaced)"""
    return s.x[OFF:OFF + n], s.y[OFF:OFF + n], (s.t_ns if t is None else t)[OFF:OFF + n]


def store_of(hip, s, n, t=None, devices=None):
    """events [0, OFF + n) of the stream in an EventStore: the first half pushed as arrays, the second as records"""
    m, t = OFF + n, s.t_ns if t is None else t
    st = hip.EventStore(W, H, 8_192, devices=devices)
    st.push(s.x[:m // 2], s.y[:m // 2], t[:m // 2])
    st.push_aos(_lib.dvs_events(s.x[m // 2:m], s.y[m // 2:m], t[m // 2:m]))
    assert (st.begin, st.end) == (0, m)
    return st


def status_of(hip, call):
    with pytest.raises(hip.CmaxHipError) as e:
        call()
    return e.value.status


@pytest.fixture(scope="module")
def fes(hip):
    out = [hip.FrontendEvaluator(W, H, packet().lut) for _ in range(3)]
    for fe in out:
        fe.set_deterministic(True)   # bitwise reproducible evaluations: any difference would be the hand-over's
    return out


@pytest.fixture(scope="module")
def bes(hip):
    out = [hip.BackendEvaluator(W, H, window().lut, WP, HP) for _ in range(3)]
    for be in out:
        be.set_deterministic(True)
    return out


@pytest.fixture(scope="module")
def grp(hip):
    return hip.BackendEvaluator(W, H, window().lut, WP, HP, devices=[0, 0, 0])


def fe_hand_over(fes, st, p, x, y, t):
    n, tail = len(x), (p.t_ref_ns, p.fx, p.fy, p.cx, p.cy, B, p.sigma, 0)
    return [lambda: fes[0].set_packet(x, y, t, *tail),
            lambda: fes[1].set_packet_aos(_lib.dvs_events(x, y, t), *tail),
            lambda: fes[2].set_packet_from(st, OFF, n, *tail)]


def be_hand_over(bes, st, w, x, y, t, rate, knots=None, t_split=None):
    n = len(x)
    t_split = int(t[n // 2]) if t_split is None else t_split   # old and new events in every window
    tail = (w.order, w.knots_init if knots is None else knots, w.start_ns, w.dt_ns, w.num_fixed, t_split, B, rate, w.sigma)
    return [lambda: bes[0].set_window(x, y, t, *tail),
            lambda: bes[1].set_window_aos(_lib.dvs_events(x, y, t), *tail),
            lambda: bes[2].set_window_from(st, OFF, n, *tail)]


def recon_add(bes, st, x, y, t):
    return [lambda: bes[0].reconstruct_add(x, y, t),
            lambda: bes[1].reconstruct_add_aos(_lib.dvs_events(x, y, t)),
            lambda: bes[2].reconstruct_add_from(st, OFF, len(x))]


@pytest.mark.parametrize("n", SIZES)
def test_frontend_packet_same_from_three_sources(hip, oracle, fes, n):
    p = packet()
    x, y, t = cut(p, n)
    for call in fe_hand_over(fes, store_of(hip, p, n), p, x, y, t):
        call()
    for om in OMEGAS:
        c0, g0 = fes[0].eval(om)
        for fe in fes[1:]:
            c, g = fe.eval(om)
            assert c == c0 and np.array_equal(g, g0), (om, c, c0, g, g0)
    if n == 4_099:
        ref = oracle.Frontend(W, H, p.lut, p.fx, p.fy, p.cx, p.cy, B, p.sigma, 0)
        ref.set_packet(x, y, t, p.t_ref_ns)
        cr, gr = ref.eval(OMEGAS[1])
        c, g = fes[2].eval(OMEGAS[1])
        print("front end, store cut vs oracle: contrast %.3e gradient %.3e" % (rel_scalar(c, cr), rel_vec(g, gr)))
        assert rel_scalar(c, cr) <= RTOL and rel_vec(g, gr) <= RTOL


@pytest.mark.parametrize("rate", RATES)
@pytest.mark.parametrize("n", SIZES)
def test_backend_window_same_from_three_sources(hip, oracle, bes, n, rate):
    w = window()
    x, y, t = cut(w, n)
    for call in be_hand_over(bes, store_of(hip, w, n), w, x, y, t, rate):
        call()
    P = 3 * (10 - w.num_fixed)
    points = [np.zeros(P), np.random.default_rng(4).normal(0, 0.01, P)]
    for d in points:
        c0, g0 = bes[0].eval(d)
        for be in bes[1:]:
            c, g = be.eval(d)
            assert c == c0 and np.array_equal(g, g0), (c, c0)
    for which in (_lib.PLANE_IL_OLD, _lib.PLANE_IL_NEW):
        ref = bes[0].get_plane(which)
        assert np.array_equal(bes[1].get_plane(which), ref) and np.array_equal(bes[2].get_plane(which), ref)
    assert bes[0].get_plane(_lib.PLANE_IL_OLD).any() == (n > 1)
    if n == 4_099:
        assert bes[0].get_plane(_lib.PLANE_IL_NEW).any()
        ref = oracle.Backend(W, H, w.lut, WP, HP, w.order, B, rate, w.sigma)
        ref.set_window(x, y, t, w.knots_init, w.start_ns, w.dt_ns, w.num_fixed, int(t[n // 2]))
        cr, gr = ref.eval(points[1])
        c, g = bes[1].eval(points[1])
        print("back end rate %d, records vs oracle: contrast %.3e gradient %.3e" % (rate, rel_scalar(c, cr), rel_vec(g, gr)))
        assert rel_scalar(c, cr) <= RTOL and rel_vec(g, gr) <= RTOL


@pytest.mark.parametrize("rate", RATES)
@pytest.mark.parametrize("n", SIZES)
def test_reconstruction_add_same_from_three_sources(hip, oracle, bes, n, rate):
    w = window()
    x, y, t = cut(w, n)
    for be in bes:
        be.reconstruct_begin(w.order, w.knots_true, w.start_ns, w.dt_ns, B, rate)
    try:
        for call in recon_add(bes, store_of(hip, w, n), x, y, t):
            call()
        plane, n_sampled, n_inside = bes[0].reconstruct_get(with_counts=True)
        assert n_sampled == recon_cases.sampled(n, B, rate) and 0 <= n_inside <= n_sampled and plane.any() == (n_inside > 0)
        for be in bes[1:]:
            p2, s2, i2 = be.reconstruct_get(with_counts=True)
            assert np.array_equal(p2, plane) and (s2, i2) == (n_sampled, n_inside)
        if n == 4_099:
            ref = oracle.Backend(W, H, w.lut, WP, HP, w.order, B, rate, sigma=0.0)
            ref.set_window(x, y, t, w.knots_true, w.start_ns, w.dt_ns, len(w.knots_true), 2 ** 62)
            want = ref.accumulate_raw(np.zeros(0))[0]
            print("reconstruction rate %d, host arrays vs oracle: %.3e" % (rate, rel_img(plane, want)))
            assert rel_img(plane, want) <= RTOL
    finally:
        for be in bes:
            be.reconstruct_end()


@pytest.mark.parametrize("rate", RATES)
@pytest.mark.parametrize("n", [129, 130])
def test_group_window_same_from_three_sources(hip, bes, grp, n, rate):
    """[0, 0, 0]: batches [0, 64), [64, 128) and the tail -- at 129 a single event no batch holds (the last member is empty), at 130
    a two-event batch"""
    w = window()
    x, y, t = cut(w, n)
    one = bes[0]
    be_hand_over(bes, None, w, x, y, t, rate)[0]()
    P = 3 * (10 - w.num_fixed)
    points = [np.zeros(P), np.random.default_rng(4).normal(0, 0.01, P)]
    want = [one.eval(d) for d in points]
    expect = []
    for r in range(3):
        beg, end = dist.batch_range(n, B, r, 3)
        if beg < end < n:
            end += 1   # the one-event rule: a member's last batch is a whole one
        expect.append(recon_cases.sampled(end - beg, B, rate))
    assert sum(expect) == recon_cases.sampled(n, B, rate) and (expect[2] == 0) == (n == 129)
    for call in be_hand_over([grp] * 3, store_of(hip, w, n, devices=[0, 0, 0]), w, x, y, t, rate):
        call()
        assert grp.group_info()["events_per_member"] == expect
        for d, (c0, g0) in zip(points, want):
            c, g = grp.eval(d)
            assert abs(c - c0) <= 1e-6 * abs(c0) and np.abs(g - g0).max() <= 1e-6 * np.abs(g0).max()   # (sums in another order)


def _assert_window_refused(hip, bes, calls, status):
    for be, call in zip(bes, calls):
        assert status_of(hip, call) == status
        assert status_of(hip, lambda: be.eval(np.zeros(be.num_params))) == _lib.ERR_STATE   # a refused window is no window


def _assert_add_refused(hip, bes, w, good, calls, status):
    """a refused add adds nothing: plane and counters stay those of the add before it"""
    for be in bes:
        be.reconstruct_begin(w.order, w.knots_true, w.start_ns, w.dt_ns, B, 3)
    try:
        for be, call in zip(bes, calls):
            be.reconstruct_add(*good)
            before = be.reconstruct_get(with_counts=True)
            assert before[1] > 0
            assert status_of(hip, call) == status
            after = be.reconstruct_get(with_counts=True)
            assert np.array_equal(after[0], before[0]) and after[1:] == before[1:]
    finally:
        for be in bes:
            be.reconstruct_end()


def test_outside_event_the_sampling_skips(hip, fes, bes):
    """rate 3 samples 64, 67, 70, ... of batch 1: event 68 is never packed, and is refused all the same.  (An EventStore refuses
    it at the push: the store cannot carry this case.)"""
    w, p, n = window(), packet(), 130
    x, y, t = cut(w, n)
    x = x.copy()
    x[68] = W
    _assert_window_refused(hip, bes, be_hand_over(bes, None, w, x, y, t, 3)[:2], _lib.ERR_EVENT_RANGE)
    _assert_add_refused(hip, bes, w, cut(w, n), recon_add(bes, None, x, y, t)[:2], _lib.ERR_EVENT_RANGE)
    for fe, call in zip(fes, fe_hand_over(fes, None, p, x, y, cut(p, n)[2])[:2]):
        assert status_of(hip, call) == _lib.ERR_EVENT_RANGE
        assert status_of(hip, lambda: fe.eval(OMEGAS[1])) == _lib.ERR_STATE
    st = hip.EventStore(W, H, 8_192)
    assert status_of(hip, lambda: st.push(x, y, t)) == _lib.ERR_EVENT_RANGE
    assert status_of(hip, lambda: st.push_aos(_lib.dvs_events(x, y, t))) == _lib.ERR_EVENT_RANGE


def test_batch_ending_before_it_starts(hip, fes, bes):
    w, p, n = window(), packet(), 130
    t = w.t_ns.copy()
    t[OFF + 64:OFF + 100] += 5 * 10**9   # batch [64, 128) of the cut now ends before it starts
    x, y, tc = cut(w, n, t)
    st = store_of(hip, w, n, t)
    _assert_window_refused(hip, bes, be_hand_over(bes, st, w, x, y, tc, 1, t_split=int(w.t_ns[OFF + 65])), _lib.ERR_TIME_ORDER)
    _assert_add_refused(hip, bes, w, cut(w, n), recon_add(bes, st, x, y, tc), _lib.ERR_TIME_ORDER)
    t = p.t_ns.copy()
    t[OFF + 64:OFF + 100] += 5 * 10**9
    x, y, tc = cut(p, n, t)
    for fe, call in zip(fes, fe_hand_over(fes, store_of(hip, p, n, t), p, x, y, tc)):
        assert status_of(hip, call) == _lib.ERR_TIME_ORDER
        assert status_of(hip, lambda: fe.eval(OMEGAS[1])) == _lib.ERR_STATE


def test_batch_time_one_interval_past_the_support(hip, oracle, bes):
    w, n = window(), 4_099
    x, y, t = cut(w, n)
    last = oracle.time_batch_ns(int(t[(n - 2) // B * B]), int(t[n - 1]))
    K = (last - w.start_ns) // w.dt_ns + w.order - 1   # the last batch needs one knot more
    assert w.order <= K < len(w.knots_init)
    st = store_of(hip, w, n)
    _assert_window_refused(hip, bes, be_hand_over(bes, st, w, x, y, t, 1, knots=w.knots_init[:K]), _lib.ERR_SPLINE_RANGE)
    for be, call in zip(bes, be_hand_over(bes, st, w, x, y, t, 1, knots=w.knots_init[:K + 1])):
        call()   # one knot more: the same window is accepted
    for be in bes:
        be.reconstruct_begin(w.order, w.knots_true[:K], w.start_ns, w.dt_ns, B, 3)
    try:
        for be, call in zip(bes, recon_add(bes, st, x, y, t)):
            be.reconstruct_add(*cut(w, 130))
            before = be.reconstruct_get(with_counts=True)
            assert status_of(hip, call) == _lib.ERR_SPLINE_RANGE
            after = be.reconstruct_get(with_counts=True)
            assert np.array_equal(after[0], before[0]) and after[1:] == before[1:] and before[1] > 0
    finally:
        for be in bes:
            be.reconstruct_end()
