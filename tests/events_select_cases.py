"""The numpy side of the event-store selection tests (tests/test_gpu_events_select.py; checked on the CPU by
tests/test_events_select_cpu.py): the predicate of cmx_events_select as include/cmax_hip.h states it, the stable compaction, the
list of cases, and a small stream with polarity and two hot pixels.

Everything is integers or one fp32 compare, so the device's store is compared with compact(...) under predicate(...) EXACTLY."""
import functools

import numpy as np

import recon_cases as rc
from cmax_slam_amd import synth

W, H = rc.SENSOR[:2]
TILE = 4096                      # events per workgroup of the mark / scatter kernels
TILE_MAX = 8192                  # the largest tile the design permits: the counts below reach every edge of any permitted tile
N_BIG = 3 * TILE_MAX + 17
COUNTS = (0, 1, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 8191, 8192, 8193, N_BIG)
SCAN_PASS = 256                  # tiles one pass of the scan kernel takes
N_SCAN = SCAN_PASS * TILE + 1    # one tile more than one pass: the smallest count at which the scan loops
N_BASE = N_BIG + 200             # events of the base stream (room for first = begin + 67 and for N_BIG after it)
HOT_SHARE = 0.04                 # of the base stream's events, from its two hot pixels together


@functools.lru_cache(maxsize=None)
def stream():
    """(x, y, t_ns, pol, is_hot, hot_xy) of the base stream: N_BASE events of synth.event_stream with two hot pixels, a random
    polarity byte per event; read-only"""
    fx, fy, cx, cy = rc.SENSOR[2:]
    T = 0.1
    s = synth.event_stream(N_BASE / T, T, W, H, fx, fy, cx, cy, seed=41, hot_pixels=2, hot_share=HOT_SHARE)
    assert len(s.x) == N_BASE
    pol = (np.random.default_rng(42).random(N_BASE) < 0.5).astype(np.uint8)
    out = (s.x, s.y, s.t_ns, pol, s.is_hot, s.hot_xy)
    for a in out:
        a.setflags(write=False)
    return out


def predicate(sel, x, y, W):
    """bool[n]: the events cmx_events_select keeps.  sel: dict with any of keep (bytes), score (float32) + min_score, flags (bytes) +
    flags_mask + flags_value (default 3, 3), pixel_keep ((H, W) or flat bytes); a criterion that is absent or None is not given."""
    n = len(x)
    k = np.ones(n, bool)
    if sel.get("keep") is not None:
        k &= np.asarray(sel["keep"]).view(np.uint8) != 0
    if sel.get("score") is not None:
        s = np.asarray(sel["score"])
        assert s.dtype == np.float32
        with np.errstate(invalid="ignore"):
            k &= s >= np.float32(sel["min_score"])  # fp32 compare; NaN: False
    if sel.get("flags") is not None:
        f = np.asarray(sel["flags"], np.uint8)
        k &= (f & np.uint8(sel.get("flags_mask", 3))) == np.uint8(sel.get("flags_value", 3))
    if sel.get("pixel_keep") is not None:
        pk = np.asarray(sel["pixel_keep"]).view(np.uint8).reshape(-1)
        k &= pk[np.asarray(y, np.int64) * W + np.asarray(x, np.int64)] != 0
    return k


def compact(arrays, keep):
    """the kept elements of every array, in order (None stays None)"""
    return tuple(None if a is None else np.asarray(a)[keep] for a in arrays)


# ---------------------------------------------------------------- keep-byte patterns at count = N_BIG
def _blocks(n, b):
    return ((np.arange(n) // b) % 2 == 0).astype(np.uint8)


def _one(n, i):
    k = np.zeros(n, np.uint8)
    k[i] = 1
    return k


# name -> (kind, keep bytes of n events); kind: "some" (keeps at least one event and drops at least one), "all", "none"
PATTERNS = {
    "all": ("all", lambda n: np.ones(n, np.uint8)),
    "none": ("none", lambda n: np.zeros(n, np.uint8)),
    "first_only": ("some", lambda n: _one(n, 0)),
    "last_only": ("some", lambda n: _one(n, n - 1)),
    "alternating": ("some", lambda n: (np.arange(n) % 2).astype(np.uint8) * 255),
    "p01": ("some", lambda n: (np.random.default_rng(1).random(n) < 0.01).astype(np.uint8)),
    "p99": ("some", lambda n: (np.random.default_rng(2).random(n) < 0.99).astype(np.uint8)),
    "blocks64": ("some", lambda n: _blocks(n, 64)),              # empty waves
    "blocks_tile": ("some", lambda n: _blocks(n, TILE)),         # empty tiles
    "blocks_tile_max": ("some", lambda n: _blocks(n, TILE_MAX)),
}


def random_keep(n, seed=0):
    return (np.random.default_rng(1000 + seed).random(n) < 0.5).astype(np.uint8)


# ---------------------------------------------------------------- criteria (on the first n events of the base stream)
def scores(n, seed=3, min_score=0.25):
    """float32 scores with every special value the compare can meet, at fixed places"""
    s = np.random.default_rng(seed).normal(0.25, 1.0, n).astype(np.float32)
    special = [np.nan, np.inf, -np.inf, -0.0, 0.0, min_score, np.nextafter(np.float32(min_score), np.float32(-1)),
               np.nextafter(np.float32(min_score), np.float32(9))]
    for i, v in enumerate(special * 3):
        s[(i * 97 + 5) % n] = v
    return s


def hot_mask():
    """(H, W) bytes: zero at exactly the two hot pixels"""
    pk = np.ones((H, W), np.uint8)
    for hx, hy in stream()[5]:
        pk[hy, hx] = 0
    return pk


def _flags(n):
    return np.random.default_rng(4).integers(0, 256, n).astype(np.uint8)  # (bits above the pair too: the mask has to hide them)


# name -> (kind, n -> sel dict)
CRITERIA = {
    "keep": ("some", lambda n: dict(keep=random_keep(n, 7))),
    "score": ("some", lambda n: dict(score=scores(n), min_score=0.25)),
    "score_zero": ("some", lambda n: dict(score=scores(n, 5, 0.0), min_score=0.0)),       # -0.0 >= 0.0 holds
    "score_neg_inf": ("some", lambda n: dict(score=scores(n), min_score=-np.inf)),      # drops the NaNs alone
    "score_nan": ("none", lambda n: dict(score=scores(n), min_score=np.nan)),
    "flags33": ("some", lambda n: dict(flags=_flags(n), flags_mask=3, flags_value=3)),
    "flags21": ("some", lambda n: dict(flags=_flags(n), flags_mask=2, flags_value=0)),
    "flags_hi": ("some", lambda n: dict(flags=_flags(n), flags_mask=0x81, flags_value=0x80)),
    "flags_any": ("all", lambda n: dict(flags=_flags(n), flags_mask=0, flags_value=0)),
    "pixel": ("some", lambda n: dict(pixel_keep=hot_mask())),
    "four": ("some", lambda n: dict(keep=random_keep(n, 8), score=scores(n), min_score=-0.5, flags=_flags(n), flags_mask=1, flags_value=1,
                                    pixel_keep=hot_mask())),
    "nothing_given": ("all", lambda n: dict()),
}
N_CRIT = 2 * TILE + 100  # events the criteria cases run on


def kept_of_case(table, name, n):
    """(kind, sel, keep bool[n]) of a case on the first n events of the base stream"""
    x, y = stream()[:2]
    kind, make = table[name]
    sel = make(n)
    if table is PATTERNS:
        sel = dict(keep=sel)
    return kind, sel, predicate(sel, x[:n], y[:n], W)
