"""The host finalize of front-end gradient evaluations (cmax_slam_amd/csrc/cmx_hostfin.hpp: which records to expect, when a record
is accepted, how the records are combined) on the CPU: tests/hostfin_host.cpp is built with the plain host compiler and run over
small case files; the combine is held against a restatement written here, bit for bit.  No GPU, no libcmaxhip.so."""
import math
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHARDS_MAX, REC_WORDS, COLS, MOMENTS = 32, 16, 6, 32   # cmx_hostfin.hpp
NONE, STALE, CHECKSUM, TORN_TAIL, TORN_HEAD, ABSENT = range(6)


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("hostfin") / "hostfin_host")
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    subprocess.run([cxx, "-O2", "-std=c++17", "-ffp-contract=off", os.path.join(ROOT, "tests", "hostfin_host.cpp"), "-o", exe], check=True)
    return exe


def make_rows(G, S, gP, mu_free, seed):
    """shard sums as a launch of G workgroups leaves them (shards without a member: zeros), and the moments of a plausible image"""
    rng = np.random.default_rng(seed)
    rows = np.zeros((SHARDS_MAX + 1, COLS))
    ncol = 2 * gP if mu_free else gP
    rows[:min(G, S), :ncol] = rng.normal(0.0, 1e3, (min(G, S), ncol)) * 10.0 ** rng.integers(-6, 3, (min(G, S), ncol))
    N = 640.0 * 480.0
    s0 = float(rng.uniform(0.5, 4.0) * N)
    rows[MOMENTS, 0] = s0
    rows[MOMENTS, 1] = float(s0 * s0 / N * rng.uniform(1.0, 3.0))
    rows[MOMENTS, 2] = float(rng.integers(0, 5000))
    return rows, N


def run(program, tmp_path, G, S, gP, mu_free, measure, ticket, rows, N, damage=NONE, damage_record=0):
    recs = np.zeros((SHARDS_MAX + 1, REC_WORDS), np.uint64)
    recs[:, :COLS] = rows.view(np.uint64)
    # words the device never writes (8..15 of every line, and the lines of shards without a member) hold junk on purpose
    recs[:, 8:] = np.uint64(0xDEADBEEF)
    fin, fout = str(tmp_path / "case.bin"), str(tmp_path / "case.out")
    with open(fin, "wb") as f:
        f.write(np.array([G, S, gP, mu_free, measure, ticket, damage, damage_record], np.int64).tobytes())
        f.write(struct.pack("<d", N))
        f.write(recs.tobytes())
    subprocess.run([program, fin, fout], check=True, timeout=60)
    raw = open(fout, "rb").read()
    head = np.frombuffer(raw[:24], np.int64)
    vals = np.frombuffer(raw[24:], np.float64)
    return {"ok": int(head[0]), "have": int(head[1]), "expected": int(head[2]), "contrast": vals[0], "mu": vals[1], "grad": vals[2:8],
            "fallback": vals[8]}


def restate(rows, S, gP, mu_free, measure, N):
    """finalize_body's expressions, one IEEE operation at a time"""
    s0, s1 = float(rows[MOMENTS, 0]), float(rows[MOMENTS, 1])
    mu = s0 / N
    if measure == 1:
        contrast = s1 / N
    else:
        var = s1 / N - mu * mu
        sd = math.sqrt(var if var >= 0 else 0.0)
        contrast = sd * sd
    ncol = 2 * gP if mu_free else gP
    cols = []
    for k in range(ncol):
        w = 0.0
        for q in range(S):
            w += float(rows[q, k])
        cols.append(w)
    grad = []
    for k in range(gP):
        s = cols[k]
        s2 = cols[gP + k] if mu_free else 0.0
        grad.append(2.0 * (s - (mu * s2 if (mu_free and measure != 1) else 0.0)) / N)
    return contrast, mu, grad


def bits(v):
    return np.asarray(v, np.float64).view(np.uint64)


@pytest.mark.parametrize("measure", [0, 1])
@pytest.mark.parametrize("mu_free", [1, 0])
@pytest.mark.parametrize("G,S", [(1, 8), (2, 8), (8, 8), (9, 8), (235, 8), (977, 8), (9, 16), (16, 16), (17, 16), (977, 16), (31, 32),
                                 (32, 32), (977, 32), (5, 1)])
def test_combine_matches_restatement(program, tmp_path, G, S, measure, mu_free):
    gP = 3
    rows, N = make_rows(G, S, gP, mu_free, seed=G * 100 + S)
    r = run(program, tmp_path, G, S, gP, mu_free, measure, ticket=41 + G, rows=rows, N=N)
    nrec = min(G, S)
    assert r["expected"] == ((1 << nrec) - 1) | (1 << MOMENTS)
    assert r["ok"] == 1 and r["have"] == r["expected"]
    contrast, mu, grad = restate(rows, S, gP, mu_free, measure, N)
    assert bits(r["contrast"]) == bits(contrast) and bits(r["mu"]) == bits(mu)
    assert np.array_equal(bits(r["grad"][:gP]), bits(grad)), (r["grad"], grad)
    assert np.all(r["grad"][gP:] == 0.0)
    assert r["fallback"] == rows[MOMENTS, 2]


def test_negative_variance_clamps(program, tmp_path):
    rows, N = make_rows(8, 8, 3, 1, seed=5)
    rows[MOMENTS, 1] = rows[MOMENTS, 0] ** 2 / N * (1.0 - 1e-12)   # rounding took E[I^2] below mu^2
    r = run(program, tmp_path, 8, 8, 3, 1, 0, ticket=7, rows=rows, N=N)
    assert r["ok"] == 1 and r["contrast"] == 0.0


@pytest.mark.parametrize("damage", [STALE, CHECKSUM, TORN_TAIL, TORN_HEAD, ABSENT])
@pytest.mark.parametrize("record", [0, 7, MOMENTS])
def test_damaged_record_is_not_accepted(program, tmp_path, damage, record):
    G, S, gP = 977, 8, 3
    rows, N = make_rows(G, S, gP, 1, seed=11)
    r = run(program, tmp_path, G, S, gP, 1, 0, ticket=1000, rows=rows, N=N, damage=damage, damage_record=record)
    assert r["ok"] == 0
    assert r["have"] == r["expected"] & ~(1 << record)   # every other record is taken, this one never
    # the same damage on a line nobody expects (a shard without a member) is not even looked at
    r = run(program, tmp_path, 2, S, gP, 1, 0, ticket=1000, rows=rows, N=N, damage=damage, damage_record=5)
    assert r["ok"] == 1 and r["have"] == 0b11 | (1 << MOMENTS)
