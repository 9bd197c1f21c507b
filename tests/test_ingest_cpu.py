"""The host ingest layer (cmax_slam_amd/csrc/cmx_ingest.hpp: batch plan, packing pass, batch-time pass, a group's cut) on the CPU:
tests/ingest_host.cpp is built with the plain host compiler and run over small case files; every output is held against a numpy
restatement written here.  No GPU, no libcmaxhip.so."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import recon_cases
from cmax_slam_amd import dist
from oracle import iwe_numpy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, ERR_SPLINE_RANGE, ERR_TIME_ORDER = 0, 4, 6   # include/cmax_hip.h
W, H, B = 240, 180, 64
ORDER, START, DT = 4, 1_000_000_000, 50_000_000
SPAN = 300_000_000   # the events lie in [START, START + SPAN): batch times reach knot interval 5, K = 10 covers them
DVS = np.dtype({"names": ["x", "y", "sec", "nsec", "polarity"], "formats": ["<u2", "<u2", "<u4", "<u4", "u1"],
                "offsets": [0, 2, 4, 8, 12], "itemsize": 16})
WIDE = np.dtype({"names": ["pad", "nsec", "sec", "y", "x"], "formats": ["<u8", "<u4", "<u4", "<u2", "<u2"],
                 "offsets": [0, 8, 12, 16, 18], "itemsize": 24})
SIZES = [0, 1, 2, 63, 64, 65, 129, 130]


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("ingest") / "ingest_host")
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    subprocess.run([cxx, "-O2", "-std=c++17", "-pthread", os.path.join(ROOT, "tests", "ingest_host.cpp"), "-o", exe], check=True)
    return exe


def events(n, seed=0):
    rng = np.random.default_rng(100 + seed)
    x = rng.integers(0, W, n).astype(np.uint16)
    y = rng.integers(0, H, n).astype(np.uint16)
    t = START + np.sort(rng.integers(0, SPAN, n)).astype(np.int64)
    return x, y, t


def t_old_of(t):
    """a time inside a batch (never at a batch boundary of B = 64)"""
    return int(t[37]) if len(t) > 37 else (int(t[len(t) // 2]) if len(t) else START)


def run(program, tmp_path, x, y, t, rate, t_old, K=10, dtype=DVS, slice_batches=2):
    n = len(x)
    rec = np.zeros(n, dtype)
    rec["x"], rec["y"], rec["sec"], rec["nsec"] = x, y, t // 10**9, t % 10**9
    off = [dtype.fields[k][1] for k in ("x", "y", "sec", "nsec")]
    head = np.array([n, B, rate, W, H, t_old, ORDER, K, START, DT, dtype.itemsize] + off + [slice_batches], np.int64)
    fin, fout = str(tmp_path / "case.bin"), str(tmp_path / "case.out")
    with open(fin, "wb") as f:
        for a in (head, x, y, t, rec):
            f.write(np.ascontiguousarray(a).tobytes())
    subprocess.run([program, fin, fout], check=True, timeout=60)
    data = np.fromfile(fout, np.int64)
    arrays, i = [], 0
    while i < len(data):
        arrays.append(data[i + 1:i + 1 + data[i]])
        i += 1 + int(data[i])
    names = ["layout_ok", "plan", "out0", "soa0", "aos0", "out1", "soa1", "aos1", "sliced_n", "sliced", "store", "store_xy", "store_t",
             "bt_err_soa", "bt_soa", "bt_err_aos", "bt_aos", "fe_err", "fe_bt", "world1", "world2", "world3", "world8"]
    assert len(arrays) == len(names)
    return dict(zip(names, arrays))


def batches(n):
    """[(beg, end)] of the reference's loop: for (beg = 0; beg < n-1; beg += B) end = (n - beg > B) ? beg + B : n"""
    return [(beg, beg + B if n - beg > B else n) for beg in range(0, n - 1, B)]


def restate_words(x, y, t, rate, t_old, flag):
    idx = np.concatenate([np.arange(b, e, rate) for b, e in batches(len(x))] + [np.zeros(0, np.int64)]).astype(np.int64)
    w = x[idx].astype(np.int64) | (y[idx].astype(np.int64) << 16)
    if flag:
        w |= (t[idx] < t_old).astype(np.int64) << 31
    return w, bool(np.any((x[idx] >= W) | (y[idx] >= H)))


def restate_times(t, spans, K):
    """(kind, at, times): the first batch in error ends the list"""
    out = []
    for beg, end in spans:
        if t[end - 1] < t[beg]:
            return ERR_TIME_ORDER, beg, out
        tb = iwe_numpy.batch_time_ns(t[beg], t[end - 1])
        st = tb - START
        if K is not None and (st < 0 or st // DT + ORDER > K):
            return ERR_SPLINE_RANGE, tb, out
        out.append(tb)
    return OK, -1, out


def check(r, x, y, t, rate, t_old, K=10, outside=False):
    n = len(x)
    assert r["layout_ok"][0] == 1
    spans = batches(n)
    nb = len(spans)
    last = spans[-1][1] - spans[-1][0] if nb else 0
    n_packed = recon_cases.sampled(n, B, rate)
    assert list(r["plan"]) == [B, rate, (B + rate - 1) // rate, nb, last, n_packed]
    for flag in (0, 1):
        want, out = restate_words(x, y, t, rate, t_old, flag)
        assert len(want) == n_packed
        assert list(r["out%d" % flag]) == [out, out] and out == outside
        assert np.array_equal(r["soa%d" % flag], want)
        assert np.array_equal(r["aos%d" % flag], r["soa%d" % flag])   # word for word
    assert r["sliced_n"][0] == n_packed and np.array_equal(r["sliced"], r["soa1"])
    bad = np.flatnonzero((x >= W) | (y >= H))
    first_bad = int(bad[0]) if len(bad) else -1
    assert list(r["store"]) == [first_bad >= 0, first_bad, first_bad]
    assert np.array_equal(r["store_xy"], x.astype(np.int64) | (y.astype(np.int64) << 16)) and np.array_equal(r["store_t"], t)
    kind, at, times = restate_times(t, spans, K)
    for v in ("soa", "aos"):
        assert list(r["bt_err_" + v]) == [kind, at]
        if kind == OK:
            assert list(r["bt_" + v]) == times
    fe_spans = [(b, min(b + B, n)) for b in range(0, n, B)]   # the front end: every event is in a batch
    fe_kind, at, times = restate_times(t, fe_spans, None)
    assert list(r["fe_err"]) == [fe_kind, at]
    if fe_kind == OK:
        assert list(r["fe_bt"]) == times
    return kind


@pytest.mark.parametrize("rate", [1, 3])
@pytest.mark.parametrize("n", SIZES)
def test_plan_words_and_batch_times(program, tmp_path, n, rate):
    x, y, t = events(n, seed=n)
    t_old = t_old_of(t)
    if n > 37:
        assert t[0] < t_old <= t[min(63, n - 1)]   # inside batch 0: both values of the flag occur
    r = run(program, tmp_path, x, y, t, rate, t_old)
    assert check(r, x, y, t, rate, t_old) == OK


@pytest.mark.parametrize("n", SIZES)
def test_members_tile_the_batches_once(program, tmp_path, n):
    x, y, t = events(n, seed=n)
    r = run(program, tmp_path, x, y, t, 3, t_old_of(t))
    nb, n_packed = int(r["plan"][3]), int(r["plan"][5])
    for world in (1, 2, 3, 8):
        rows = r["world%d" % world].reshape(world, 6)
        done = 0   # batches owned by the members before this one
        for rank, (b0, b1, m0, m1, m_nb, m_packed) in enumerate(rows):
            assert (b0, b1) == dist.batch_range(n, B, rank, world)
            assert (m0, m1) == (b0, b1 + 1 if b0 < b1 < n else b1)   # one event more than the member's batches hold
            if m_nb:
                assert m0 == done * B   # its batches start where the previous member's end
            done += int(m_nb)
        assert done == nb and rows[:, 5].sum() == n_packed
        if world == 8:
            assert (rows[:, 3] == rows[:, 2]).any()   # some member comes out empty


def test_outside_event_the_sampling_skips(program, tmp_path):
    x, y, t = events(130, seed=1)
    x = x.copy()
    x[64 + 4] = W   # batch 1 samples 64, 67, 70, ...: the packing pass at rate 3 never reads it
    r = run(program, tmp_path, x, y, t, 3, t_old_of(t))
    assert list(r["out0"]) == [0, 0] and list(r["store"])[1:] == [68, 68]
    check(r, x, y, t, 3, t_old_of(t))
    r = run(program, tmp_path, x, y, t, 1, t_old_of(t))
    check(r, x, y, t, 1, t_old_of(t), outside=True)


@pytest.mark.parametrize("rate", [1, 3])
def test_batch_ending_before_it_starts(program, tmp_path, rate):
    x, y, t = events(130, seed=2)
    t = t.copy()
    t[64:100] += 5 * 10**9   # batch [64, 128) now ends before it starts
    r = run(program, tmp_path, x, y, t, rate, t_old_of(t))
    assert check(r, x, y, t, rate, t_old_of(t)) == ERR_TIME_ORDER
    assert list(r["bt_err_soa"]) == [ERR_TIME_ORDER, 64]


def test_batch_time_one_interval_past_the_support(program, tmp_path):
    x, y, t = events(130, seed=3)
    last = iwe_numpy.batch_time_ns(t[128], t[129])
    K = (last - START) // DT + ORDER - 1   # the last batch needs one knot more
    r = run(program, tmp_path, x, y, t, 1, t_old_of(t), K=int(K))
    assert check(r, x, y, t, 1, t_old_of(t), K=int(K)) == ERR_SPLINE_RANGE
    assert list(r["bt_err_aos"]) == [ERR_SPLINE_RANGE, last]
    r = run(program, tmp_path, x, y, t, 1, t_old_of(t), K=int(K) + 1)
    assert check(r, x, y, t, 1, t_old_of(t), K=int(K) + 1) == OK


@pytest.mark.parametrize("rate", [1, 3])
def test_wide_record(program, tmp_path, rate):
    x, y, t = events(130, seed=4)
    r = run(program, tmp_path, x, y, t, rate, t_old_of(t), dtype=WIDE)
    assert check(r, x, y, t, rate, t_old_of(t)) == OK


@pytest.mark.parametrize("rate", [1, 3])
def test_pool_path_equals_the_single_range(program, tmp_path, rate):
    n = 300_000   # above parallel_ranges' serial threshold (262 144): the flat pass runs on the host pool
    x, y, t = events(n, seed=5)
    t_old = int(t[n // 2 + 17])
    r = run(program, tmp_path, x, y, t, rate, t_old, slice_batches=2048)   # slices of 131 072 events: each a single range
    assert check(r, x, y, t, rate, t_old) == OK


def test_the_slice_planner_against_brute_force(tmp_path):
    """feed_slice_at alone (the slices of every cmx_backend_recon_add* / _grad_add* / _warp* call), under the address and
    undefined-behaviour sanitizers, run directly: every n in 0 .. 3 B + 2 with B in {1, 3, 64}, rates 1 to 3, 1, 2 and 7 batches per
    slice, the sampling mode and the export's "every event, lone tail included" (tests/feed_plan_host.cpp)."""
    exe = str(tmp_path / "feed_plan_host")
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "feed_plan_host.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and r.stdout.startswith("ok ")
