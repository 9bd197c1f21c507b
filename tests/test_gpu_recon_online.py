"""GPU: a whole-trajectory binding that grows (cmx_backend_recon_extend / _bind_append_from / _advance_head / _release_head /
_online_info, cmx_backend_recon_solve with CMX_RECON_KEEP_HEAD; BackendEvaluator.reconstruct_extend / _bind_append / _advance_head /
_release_head / _online_info, reconstruct_solve(freeze_head="keep")).

Reference, in deterministic mode: a FRESH context that begins with the knots of the moment, binds everything bound so far with one
bind_from and freezes with one freeze_head -- plane bytes, both counters, the contrast and the gradient must be equal bit for bit
(frozen batches read only knots whose bytes never changed, fixed-point adds commute, and the gather pass starts at the same batch).
In default mode the CPU oracle's global_contrast_fdf with num_fixed (recon_grad_cases.oracle_eval) at RTOL.  The schedules are
tests/recon_online_cases.py's; tests/test_recon_online_cpu.py checks the planner and the schedules on the CPU."""
import numpy as np
import pytest

import recon_cases as rc
import recon_grad_cases as rg
import recon_online_cases as ro
from cmax_slam_amd import _lib
from cmax_slam_amd._lib import CmaxHipError
from test_gpu_recon_bound import W, H, bound, make, store_of
from util import RTOL, rel_scalar, rel_vec

pytestmark = pytest.mark.gpu

NO_HEAD = {"num_fixed": 0, "frozen_batches": 0, "frozen_sampled": 0}


def begin(be, name, q):
    c, w = rc.CASES[name], rc.window(name)[0]
    be.reconstruct_begin(c["order"], q, w.start_ns, w.dt_ns, c["batch"], c["rate"])


def status_of(call, *args, **kw):
    with pytest.raises(CmaxHipError) as e:
        call(*args, **kw)
    return e.value.status


def equal_bits(tag, got, want):
    """(contrast, gradient, plane bytes, n_sampled, n_inside) of two evaluations, bit for bit"""
    print("%s: contrast %.10g / %.10g, sampled %d / %d, inside %d / %d, |g|max %.4g / %.4g" %
          (tag, got[0], want[0], got[3], want[3], got[4], want[4], np.abs(got[1]).max(), np.abs(want[1]).max()))
    assert got[3:] == want[3:], tag
    assert got[2] == want[2], tag + ": plane bytes differ"
    assert got[0] == want[0], tag
    assert got[1].tobytes() == want[1].tobytes(), tag + ": gradient bytes differ"


_fresh = {}


def fresh(hip, name, n, q, nf, key=None):
    """the from-scratch result: begin(q) + bind_from(the first n events) + freeze_head(nf), evaluated at q (computed once per key)"""
    if key is not None and (name,) + key in _fresh:
        return _fresh[(name,) + key]
    be = make(hip, name, deterministic=True)
    store = store_of(hip, name)
    begin(be, name, q)
    be.reconstruct_bind(store, 0, n)
    if nf:
        be.reconstruct_freeze_head(nf)
    out = (bound(be, q), be.reconstruct_frozen_info(), be.reconstruct_bound_info())
    assert out[0][4] > 0 and np.abs(out[0][1]).max() > 0  # events vote, the gradient is not zero
    be.reconstruct_end()
    store.close()
    if key is not None:
        _fresh[(name,) + key] = out
    return out


def counts_of(info):
    return {k: info[k] for k in ("n_events", "n_sampled")}


# ---------------------------------------------------------------- 1. append equals bind
def append_cuts(name):
    """a batch multiple, mid-batch, one event past a multiple"""
    c = rc.CASES[name]
    N, B = c["N"], c["batch"]
    full = N // B
    cuts = [max(full // 4, 1) * B, max(full // 2, 1) * B + B // 2, max(3 * full // 4, 2) * B + 1]
    assert 0 < cuts[0] < cuts[1] < cuts[2] < N and cuts[0] % B == 0 and cuts[2] % B == 1 % B
    return cuts


def appended(hip, name, edges, q, drop=False):
    """bind [edges[0], edges[1]), append the following ranges; the evaluation at q and the counts"""
    be = make(hip, name, deterministic=True)
    store = store_of(hip, name)
    begin(be, name, q)
    be.reconstruct_bind(store, edges[0], edges[1] - edges[0])
    for lo, hi in zip(edges[1:-1], edges[2:]):
        if drop:
            store.drop_before(lo)  # (the events bound so far are gone from the store)
        be.reconstruct_bind_append(store, lo, hi - lo)
    assert be.reconstruct_online_info() == {"released_batches": 0, "released_events": 0, "released_sampled": 0,
                                            "resident_sampled": be.reconstruct_bound_info()["n_sampled"]}
    out = bound(be, q), counts_of(be.reconstruct_bound_info())
    again = bound(be, q)  # (the second evaluation keeps the sort: the same bits)
    equal_bits(name + " again", again, out[0])
    be.reconstruct_end()
    store.close()
    return out


@pytest.mark.parametrize("name,drop", [(n, False) for n in ro.SCHEDULES] + [("B", True), ("batch3", True)])
def test_append_equals_bind(hip, name, drop):
    c, q = rc.CASES[name], rg.point(name)
    want, _, winfo = fresh(hip, name, c["N"], q, 0, key=("all",))
    got, ginfo = appended(hip, name, [0] + append_cuts(name) + [c["N"]], q, drop)
    equal_bits("%s cut at %s%s" % (name, append_cuts(name), " (dropped)" if drop else ""), got, want)
    assert ginfo == counts_of(winfo) and ginfo["n_sampled"] == rc.sampled(c["N"], c["batch"], c["rate"])


@pytest.mark.parametrize("edges", [[0, 64, 65], [0, 65, 65], [0, 1, 65], [0, 0, 1, 2, 65], [0, 2, 64, 65]])
def test_append_around_one_batch(hip, edges):
    """n65: one batch of 64 and a lone trailing event -- bind 64 + 1, 65 + 0, 1 + 64, and from nothing"""
    name = "n65"
    q = rg.point(name)
    want, _, winfo = fresh(hip, name, 65, q, 0, key=("all",))
    got, ginfo = appended(hip, name, edges, q)
    equal_bits("n65 %s" % edges, got, want)
    assert ginfo == counts_of(winfo) == {"n_events": 65, "n_sampled": 64}


def test_append_validation_leaves_the_binding(hip):
    name = "B"
    c, q = rc.CASES[name], rg.point(name)
    _, x, y, t = rc.window(name)
    be = make(hip, name, deterministic=True)
    store = store_of(hip, name)
    begin(be, name, q)
    assert status_of(be.reconstruct_bind_append, store, 0, 10) == _lib.ERR_STATE  # no binding
    assert be.reconstruct_online_info() == {"released_batches": 0, "released_events": 0, "released_sampled": 0, "resident_sampled": 0}
    be.reconstruct_bind(store, 1000, 5000)
    before, info = bound(be, q), be.reconstruct_bound_info()
    assert t[999] < t[5999]
    assert status_of(be.reconstruct_bind_append, store, 999, 10) == _lib.ERR_TIME_ORDER  # earlier than the last bound event
    assert status_of(be.reconstruct_bind_append, store, 6000, c["N"]) == _lib.ERR_INVALID_ARG  # not held by the store
    assert status_of(be.reconstruct_bind_append, store, 6000, -1) == _lib.ERR_INVALID_ARG
    assert counts_of(be.reconstruct_bound_info()) == counts_of(info)
    equal_bits("after refused appends", bound(be, q), before)
    be.reconstruct_contrast(want_grad=True)  # count == 0: valid, closes an open gradient pass, changes nothing else
    be.reconstruct_bind_append(store, 6000, 0)
    assert status_of(be.reconstruct_grad_get) == _lib.ERR_STATE
    assert counts_of(be.reconstruct_bound_info()) == counts_of(info)
    equal_bits("after an empty append", bound(be, q), before)
    be.reconstruct_end()
    store.close()


# ---------------------------------------------------------------- 2. extend
def test_extend_then_append(hip):
    name = "A"
    c, q = rc.CASES[name], rg.point(name)
    K1 = 40
    n1 = ro.cut(name, K1)
    q1 = np.ascontiguousarray(q[:K1])
    want, _, winfo = fresh(hip, name, c["N"], q, 0, key=("all",))
    be = make(hip, name, deterministic=True)
    store = store_of(hip, name)
    begin(be, name, q1)
    be.reconstruct_bind(store, 0, n1)
    before = bound(be, q1)
    assert before[4] > 0
    # past the support of the K1 knots: judged against the K of this moment
    assert status_of(be.reconstruct_bind_append, store, n1, c["N"] - n1) == _lib.ERR_SPLINE_RANGE
    assert be.reconstruct_bound_info()["n_events"] == n1
    equal_bits("after the refused append", bound(be, q1), before)
    assert status_of(be.reconstruct_extend, q1[:K1 - 1]) == _lib.ERR_INVALID_ARG  # shorter
    equal_bits("after the refused extend", bound(be, None), before)
    be.reconstruct_extend(q)
    assert be.reconstruct_get(with_counts=True)[1:] == (0, 0) and not be.reconstruct_get().any()  # plane and counters start over
    be.reconstruct_bind_append(store, n1, c["N"] - n1)
    got = bound(be, q)
    equal_bits("extend 40 -> 100 + append", got, want)
    assert counts_of(be.reconstruct_bound_info()) == counts_of(winfo)
    # K_new == K without a frozen head: restart
    be.reconstruct_extend(q)
    equal_bits("extend at the same K", bound(be, None), want)
    # under a frozen head the fixed knots keep their bytes
    nf = 50
    be.reconstruct_freeze_head(nf)
    frozen, info = bound(be, q), be.reconstruct_frozen_info()
    assert info["frozen_batches"] > 0
    moved = np.array(q, copy=True)
    moved[10] = rg.perturb(q[10:11], 99)[0]
    assert status_of(be.reconstruct_extend, moved) == _lib.ERR_INVALID_ARG
    assert be.reconstruct_frozen_info() == info
    equal_bits("after the refused extend under a head", bound(be, None), frozen)
    free = np.array(q, copy=True)
    free[nf:] = rg.perturb(q[nf:], 98, ro.MOVE)
    be.reconstruct_extend(free)  # the free knots may move: the head survives
    assert be.reconstruct_frozen_info() == info
    want_free, winfo_free, _ = fresh(hip, name, c["N"], np.ascontiguousarray(free), nf)
    equal_bits("extend under a head, free knots moved", bound(be, None), want_free)
    assert winfo_free == info
    be.reconstruct_end()
    store.close()


# ---------------------------------------------------------------- 3. advance, 4. release
def run_schedule(hip, name, release, deterministic=True, steps=None, after_step=None):
    """the online loop over the schedule: extend, append, evaluate at the moved knots, advance [, release], evaluate again"""
    c = rc.CASES[name]
    be = make(hip, name, deterministic=deterministic)
    store = store_of(hip, name)
    sched = ro.SCHEDULES[name]
    prev_n, prev_nf = 0, 0
    for i, (K, nf) in enumerate(sched[:steps]):
        q, n = ro.knots(name)[i], ro.cut(name, K)
        if i == 0:
            begin(be, name, q)
            be.reconstruct_bind(store, 0, n)
        else:
            be.reconstruct_extend(q)
            be.reconstruct_bind_append(store, prev_n, n - prev_n)
        mid = bound(be, q)
        if prev_nf:
            assert status_of(be.reconstruct_advance_head, prev_nf - 1) == _lib.ERR_INVALID_ARG  # going back is freeze_head's job
        assert status_of(be.reconstruct_advance_head, K) == _lib.ERR_INVALID_ARG
        be.reconstruct_advance_head(nf)
        if release:
            be.reconstruct_release_head()
        got = bound(be, q)
        if after_step:
            after_step(be, i, K, nf, prev_nf, n, q, mid, got)
        prev_n, prev_nf = n, nf
    return be, store


def check_step(hip, name, release):
    c = rc.CASES[name]

    def after(be, i, K, nf, prev_nf, n, q, mid, got):
        tag = "%s step %d (K %d, num_fixed %d, %d events)%s" % (name, i, K, nf, n, " released" if release else "")
        want_mid, _, _ = fresh(hip, name, n, q, prev_nf, key=(i, prev_nf))
        equal_bits(tag + " before the advance", mid, want_mid)
        want, winfo, wbound = fresh(hip, name, n, q, nf, key=(i, nf))
        equal_bits(tag, got, want)
        assert not got[1][:3 * nf].any()
        info = be.reconstruct_frozen_info()
        assert info == winfo and info["num_fixed"] == nf
        fb, nb = ro.frozen_batches(name, n, K, nf)
        assert info["frozen_batches"] == fb and info["frozen_sampled"] == ro.sampled_in(name, n, fb)
        assert counts_of(be.reconstruct_bound_info()) == counts_of(wbound)  # the totals since the bind
        on = be.reconstruct_online_info()
        if release:
            assert on == {"released_batches": fb, "released_events": fb * c["batch"], "released_sampled": info["frozen_sampled"],
                          "resident_sampled": wbound["n_sampled"] - info["frozen_sampled"]}
            assert on["resident_sampled"] > 0
        else:
            assert on == {"released_batches": 0, "released_events": 0, "released_sampled": 0, "resident_sampled": wbound["n_sampled"]}
        equal_bits(tag + " again", bound(be, q), want)
    return after


@pytest.mark.parametrize("name", list(ro.SCHEDULES))
def test_advance_equals_a_fresh_freeze(hip, name):
    be, store = run_schedule(hip, name, release=False, after_step=check_step(hip, name, False))
    be.reconstruct_end()
    store.close()


@pytest.mark.parametrize("name", list(ro.SCHEDULES))
def test_release_changes_no_evaluation(hip, name):
    be, store = run_schedule(hip, name, release=True, after_step=check_step(hip, name, True))
    # what would lose the released events is refused, and changes nothing
    K, nf = ro.SCHEDULES[name][-1]
    q, n = ro.knots(name)[-1], rc.CASES[name]["N"]
    want = fresh(hip, name, n, q, nf, key=(len(ro.SCHEDULES[name]) - 1, nf))
    info, on = be.reconstruct_frozen_info(), be.reconstruct_online_info()
    assert status_of(be.reconstruct_restart, q) == _lib.ERR_STATE
    assert status_of(be.reconstruct_freeze_head, 0) == _lib.ERR_STATE
    assert status_of(be.reconstruct_freeze_head, nf) == _lib.ERR_STATE
    assert status_of(be.reconstruct_eval, store, 0, n, knots=q) == _lib.ERR_STATE
    assert status_of(be.reconstruct_solve, q, nf, freeze_head=False, max_iterations=1) == _lib.ERR_STATE
    assert status_of(be.reconstruct_solve, q, nf, freeze_head=True, max_iterations=1) == _lib.ERR_STATE
    assert be.reconstruct_frozen_info() == info and be.reconstruct_online_info() == on
    equal_bits(name + " after the refused calls", bound(be, q), want[0])
    be.reconstruct_release_head()  # nothing new to give back: valid
    assert be.reconstruct_online_info() == on
    # unbind and bind_from work, and drop everything
    be.reconstruct_unbind()
    assert be.reconstruct_frozen_info() == NO_HEAD and not any(be.reconstruct_online_info().values())
    be.reconstruct_bind(store, 0, n)
    assert be.reconstruct_online_info()["released_sampled"] == 0 and be.reconstruct_frozen_info() == NO_HEAD
    be.reconstruct_restart(q)
    all_want = fresh(hip, name, n, q, 0, key=("last", 0))
    equal_bits(name + " bound again", bound(be, q), all_want[0])
    be.reconstruct_end()
    store.close()


def test_resident_events_follow_the_active_tail(hip):
    """released, then appended to: the resident count follows the active tail, not the recording"""
    name = "batch1"
    seen = []
    be, store = run_schedule(hip, name, release=True,
                             after_step=lambda be, i, K, nf, prev_nf, n, q, mid, got: seen.append(be.reconstruct_online_info()))
    total = be.reconstruct_bound_info()["n_sampled"]
    assert [s["released_sampled"] for s in seen] == sorted(s["released_sampled"] for s in seen)
    assert all(s["resident_sampled"] + s["released_sampled"] == ro.sampled_in(name, ro.cut(name, K), 10 ** 9)
               for s, (K, _) in zip(seen, ro.SCHEDULES[name]))
    assert max(s["resident_sampled"] for s in seen) < 0.6 * total
    be.reconstruct_end()
    store.close()


# ---------------------------------------------------------------- 5. solve under the head as it stands
def test_solve_keeps_the_head(hip):
    name = "B"
    c = rc.CASES[name]
    sched = ro.SCHEDULES[name]
    be, store = run_schedule(hip, name, release=True, steps=2)
    (K, _), nf = sched[2], sched[1][1]
    q, n = ro.knots(name)[2], c["N"]
    be.reconstruct_extend(q)
    be.reconstruct_bind_append(store, ro.cut(name, sched[1][0]), n - ro.cut(name, sched[1][0]))
    head = be.reconstruct_frozen_info()
    assert head["num_fixed"] == nf and be.reconstruct_online_info()["released_batches"] == head["frozen_batches"] > 0
    assert status_of(be.reconstruct_solve, q, nf + 1, freeze_head="keep", max_iterations=4) == _lib.ERR_INVALID_ARG
    moved = np.array(q, copy=True)
    moved[0] = rg.perturb(q[:1], 97)[0]
    assert status_of(be.reconstruct_solve, moved, nf, freeze_head="keep", max_iterations=4) == _lib.ERR_INVALID_ARG
    knots, rep = be.reconstruct_solve(q, nf, freeze_head="keep", max_iterations=4)
    counts = be.reconstruct_solve_counts()
    assert be.reconstruct_frozen_info() == head
    ref = make(hip, name, deterministic=True)
    begin(ref, name, q)
    ref.reconstruct_bind(store, 0, n)
    assert status_of(ref.reconstruct_solve, q, nf, freeze_head="keep", max_iterations=4) == _lib.ERR_STATE  # no head to keep
    want_knots, want_rep = ref.reconstruct_solve(q, nf, freeze_head=True, max_iterations=4)
    print("solve: %s / %s, evaluations %s / %s, moved %.3g deg" % (rep, want_rep, counts, ref.reconstruct_solve_counts(),
                                                                 rg.rms_angle_deg(q, knots)))
    assert knots.tobytes() == want_knots.tobytes()
    assert rep == want_rep and rep["iterations"] > 0 and counts[0] == ref.reconstruct_solve_counts()[0]
    assert knots[:nf].tobytes() == q[:nf].tobytes() and not np.array_equal(knots[nf:], q[nf:])
    ref.reconstruct_end()
    be.reconstruct_end()
    store.close()


# ---------------------------------------------------------------- 6. default mode against the oracle
@pytest.mark.parametrize("name", ["A", "B"])
def test_default_mode_against_the_oracle(hip, oracle, name):
    _, x, y, t = rc.window(name)

    def after(be, i, K, nf, prev_nf, n, q, mid, got):
        for tag, ev, f in (("before the advance", mid, prev_nf), ("advanced and released", got, nf)):
            cr, gr = rg.oracle_eval(oracle, name, x[:n], y[:n], t[:n], q, 1.0, 0, num_fixed=f)
            ec, eg = rel_scalar(ev[0], cr), rel_vec(ev[1][3 * f:], gr)
            print("%s step %d %s: contrast %.8g (oracle %.8g, rel %.2e), gradient rel %.2e" % (name, i, tag, ev[0], cr, ec, eg))
            assert ec < RTOL and eg < RTOL
            assert not ev[1][:3 * f].any()
    be, store = run_schedule(hip, name, release=True, deterministic=False, after_step=after)
    be.reconstruct_end()
    store.close()


# ---------------------------------------------------------------- 7. a frozen open batch
def test_an_append_that_cuts_a_frozen_batch_again_is_refused(hip):
    """the recording ends early, all knots but the last are fixed: every batch is frozen, the open last one included"""
    name = "A"
    c, q = rc.CASES[name], rg.point(name)
    n, nf = c["N"] // 2, c["K"] - 1
    assert n % c["batch"] not in (0, 1) and ro.frozen_batches(name, n, c["K"], nf) == (n // c["batch"] + 1,) * 2
    be = make(hip, name, deterministic=True)
    store = store_of(hip, name)
    begin(be, name, q)
    be.reconstruct_bind(store, 0, n)
    be.reconstruct_advance_head(nf)  # (without a head: freeze_head)
    before, info, binfo = bound(be, q), be.reconstruct_frozen_info(), be.reconstruct_bound_info()
    assert info["frozen_batches"] == n // c["batch"] + 1
    assert status_of(be.reconstruct_bind_append, store, n, 500) == _lib.ERR_STATE
    assert be.reconstruct_frozen_info() == info and counts_of(be.reconstruct_bound_info()) == counts_of(binfo)
    equal_bits("after the refused append", bound(be, q), before)
    be.reconstruct_end()
    store.close()
