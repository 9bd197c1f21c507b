"""The host packing with polarity (cmax_slam_amd/csrc/cmx_ingest.hpp: pack_events<false, true>, pack_polarity, aos_view_pol) on the
CPU: tests/pol_pack_host.cpp is built with the plain host compiler -- and once more with -fsanitize=address,undefined -- and run
over small case files; every output is held against a numpy restatement written here.  No GPU, no libcmaxhip.so.

The packed word of a polarity hand-over is x | y << 16 | (polarity != 0) << 31: bit 31 is the bit the reconstruction kernels mask
off before they read the coordinates, so the host paths of cmx_backend_recon_pol_add* upload nothing beside the words."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, B = 240, 180, 64
START, SPAN = 1_000_000_000, 300_000_000
DVS = np.dtype({"names": ["x", "y", "sec", "nsec", "polarity"], "formats": ["<u2", "<u2", "<u4", "<u4", "u1"],
                "offsets": [0, 2, 4, 8, 12], "itemsize": 16})
WIDE = np.dtype({"names": ["pad", "nsec", "sec", "y", "x", "polarity"], "formats": ["<u8", "<u4", "<u4", "<u2", "<u2", "u1"],
                 "offsets": [0, 8, 12, 16, 18, 23], "itemsize": 24})   # (the polarity in the record's last byte)
SIZES = [0, 1, 2, 63, 64, 65, 129, 130]
BUILDS = {"plain": ["-O2"], "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}


@pytest.fixture(scope="module", params=list(BUILDS))
def program(request, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("polpack") / ("pol_pack_host_" + request.param))
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    subprocess.run([cxx] + BUILDS[request.param] + ["-std=c++17", "-pthread", os.path.join(ROOT, "tests", "pol_pack_host.cpp"), "-o", exe],
                   check=True)
    return exe


def events(n, seed=0):
    rng = np.random.default_rng(300 + seed)
    x = rng.integers(0, W, n).astype(np.uint16)
    y = rng.integers(0, H, n).astype(np.uint16)
    t = START + np.sort(rng.integers(0, SPAN, n)).astype(np.int64)
    pol = rng.choice(np.array([0, 1, 1, 2, 255], np.uint8), n)   # any nonzero byte is ON
    return x, y, t, pol


def run(program, tmp_path, x, y, t, pol, rate, dtype, slice_batches=2):
    n = len(x)
    rec = np.zeros(n, dtype)
    rec["x"], rec["y"], rec["sec"], rec["nsec"], rec["polarity"] = x, y, t // 10**9, t % 10**9, pol
    off = [dtype.fields[k][1] for k in ("x", "y", "sec", "nsec", "polarity")]
    head = np.array([n, B, rate, W, H, dtype.itemsize] + off + [slice_batches], np.int64)
    fin, fout = str(tmp_path / "case.bin"), str(tmp_path / "case.out")
    with open(fin, "wb") as f:
        for a in (head, x, y, t, pol, rec):
            f.write(np.ascontiguousarray(a).tobytes())
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    done = subprocess.run([program, fin, fout], timeout=60, env=env, capture_output=True, text=True)
    assert done.returncode == 0 and "runtime error" not in done.stderr and "Sanitizer" not in done.stderr, done.stderr
    data = np.fromfile(fout, np.int64)
    arrays, i = [], 0
    while i < len(data):
        arrays.append(data[i + 1:i + 1 + data[i]])
        i += 1 + int(data[i])
    names = ["layout", "plan", "outside", "soa", "aos", "plain", "sliced_n", "sliced", "bytes_soa", "bytes_aos"]
    assert len(arrays) == len(names)
    return dict(zip(names, arrays))


def batches(n):
    """[(beg, end)] of the reference's loop: for (beg = 0; beg < n-1; beg += B) end = (n - beg > B) ? beg + B : n"""
    return [(beg, beg + B if n - beg > B else n) for beg in range(0, n - 1, B)]


def restate(x, y, pol, rate):
    """(words with the polarity bit, words without) of the sampled events: every rate-th event from its batch's start"""
    idx = np.concatenate([np.arange(b, e, rate) for b, e in batches(len(x))] + [np.zeros(0, np.int64)]).astype(np.int64)
    plain = x[idx].astype(np.int64) | (y[idx].astype(np.int64) << 16)
    return plain | ((pol[idx] != 0).astype(np.int64) << 31), plain


@pytest.mark.parametrize("dtype", [DVS, WIDE], ids=["dvs", "wide"])
@pytest.mark.parametrize("rate", [1, 3])
@pytest.mark.parametrize("n", SIZES)
def test_packed_words_carry_the_polarity_in_bit_31(program, tmp_path, n, rate, dtype):
    x, y, t, pol = events(n, seed=n + rate)
    r = run(program, tmp_path, x, y, t, pol, rate, dtype)
    assert list(r["layout"]) == [1, 0, 1]
    want, plain = restate(x, y, pol, rate)
    assert list(r["plan"]) == [len(batches(n)), len(want)]
    assert list(r["outside"]) == [0, 0, 0]
    assert np.array_equal(r["soa"], want) and np.array_equal(r["aos"], want)
    assert np.array_equal(r["plain"], plain) and not (r["plain"] >> 31).any()
    assert np.array_equal(r["soa"] & 0x7fffffff, plain)                       # what the kernels read as coordinates
    assert r["sliced_n"][0] == len(want) and np.array_equal(r["sliced"], want)  # the feeder's slices of two batches
    assert np.array_equal(r["bytes_soa"], (pol != 0).astype(np.int64)) and np.array_equal(r["bytes_aos"], r["bytes_soa"])
    if n >= 63:   # both polarities occur among the sampled events: neither comparison above is an empty one
        assert (r["soa"] >> 31).any() and not (r["soa"] >> 31).all()


def test_dvs_polarity_offset_matches_the_header():
    text = open(os.path.join(ROOT, "include", "cmax_hip.h")).read()
    assert "#define CMX_AOS_DVS_POLARITY 12" in text and DVS.fields["polarity"][1] == 12
