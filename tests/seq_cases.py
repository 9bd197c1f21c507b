"""Test helper (no HIP): sparse scenes and seeded call sequences for tests/test_gpu_call_sequences.py.

A context keeps state between calls -- two ping-pong vote planes with their clean flags, the ids of the sort the votes were made
under, the fallback share and reach flags of the last collected evaluation, a resident image and its Jt, the warm end of a
device-driven solve.  The oracle keeps none of it in anything the front end returns, so the model of a stateful test is free:
whatever a context did before, call k returns what the oracle returns for call k's arguments.

Everything here is chosen from the oracle alone (numpy, cmax_slam_amd.synth, oracle/): the packets, the points, the operation
lists and the expected values.  tests/test_seq_cases_cpu.py checks the properties the GPU tests rely on.

Front-end scenes (240 x 180, fx = fy = 200): 20 000 events in a corner of the image, 98 % of them within 1 ms of the
reference time and 2-3 % at 20-50 ms.  A step of 12 rad/s in omega moves the many by under 3 px and carries the few over
100 px, into 32 x 32 tiles that are inactive under the sort of the step's starting point and out of reach of every chunk
(kFuseNbr = 2 tiles): the fallback share stays at or under kRebinFallbackFrac = 3 % (no new sort), and the votes lie where only
a whole-plane clear removes them."""
import functools

import numpy as np

from cmax_slam_amd import synth
from oracle import pyoracle as po

W, H = 240, 180
FX = FY = 200.0
CX, CY = 119.5, 89.5
TILE = 32            # kBinTile: side of a sort tile and of a fused image-pass tile
BIN_MARGIN = 16      # kBinMargin: the LDS window is the tile and this many pixels on every side
FUSE_NBR = 2         # kFuseNbr: a chunk arrives on the tiles up to this many away from its own
FUSE_REACH = FUSE_NBR * TILE - 8   # kFuseReach: how far from its tile a vote may land and still be covered by those arrivals
REBIN_FRAC = 0.03    # kRebinFallbackFrac
T_REF_NS = synth.T0_NS + 60_000_000
OMEGA0 = np.array([0.3, -0.5, 0.2])
EPS = np.array([0.02, -0.03, 0.01])   # a "near" step: under 0.1 px for every event of the sparse packets


# ------------------------------------------------------------------------------------------------- front-end packets
def _sparse(seed, groups, mirror):
    """groups: ((share, lo_ms, hi_ms[, signs]), ...) of events at +-lo..hi ms from the reference time; the rest within +-1 ms."""
    rng = np.random.default_rng(seed)
    n = 20_000
    x = np.clip(np.rint(rng.normal(16, 5, n)), 2, 30).astype(np.int64)
    y = np.clip(np.rint(rng.normal(16, 5, n)), 2, 30).astype(np.int64)
    y[rng.random(n) < 0.4] += 96
    dt = rng.uniform(-1e-3, 1e-3, n)
    u = rng.random(n)
    lo = 0.0
    for share, a_ms, b_ms, *signs in groups:
        m = (u >= lo) & (u < lo + share)
        dt[m] = rng.choice(signs[0] if signs else [-1.0, 1.0], int(m.sum())) * rng.uniform(a_ms * 1e-3, b_ms * 1e-3, int(m.sum()))
        lo += share
    if mirror:   # bottom-right corner: next to the image border and in the ragged last tile row (180 = 5 * 32 + 20)
        x, y = W - 1 - x, H - 1 - y
    o = np.argsort(dt, kind="stable")
    t = T_REF_NS + np.rint(dt[o] * 1e9).astype(np.int64)
    return synth.FrontendPacket(W, H, FX, FY, CX, CY, x[o].astype(np.uint16), y[o].astype(np.uint16), t, T_REF_NS, np.zeros(3))


@functools.lru_cache(maxsize=None)
def packet(name):
    """'A' the basic recipe, 'B' its mirror image in the bottom-right corner, 'C' two far groups at different |dt|, 'D' dense."""
    if name == "A":
        return _sparse(11, ((0.02, 45, 50),), False)
    if name == "B":
        return _sparse(12, ((0.02, 45, 50),), True)
    if name == "C":
        return _sparse(13, ((0.014, 45, 50, [1.0]), (0.010, 20, 25)), False)   # (the far group after the reference time only)
    if name == "D":
        return synth.frontend_packet(20_000, W, H, FX, FY, CX, CY, seed=14)
    raise KeyError(name)


SPARSE = ("A", "B", "C")
PACKETS = SPARSE + ("D",)


@functools.lru_cache(maxsize=None)
def fe_oracle(name):
    p = packet(name)
    ref = po.Frontend(p.W, p.H, p.lut, p.fx, p.fy, p.cx, p.cy, p.batch, p.sigma, po.VARIANCE)
    ref.set_packet(p.x, p.y, p.t_ns, p.t_ref_ns)
    return ref


def positions(p, omega):
    """Real-valued warped position (u, v) of every event: oracle/iwe_numpy.py's front-end warp without the votes."""
    from oracle import iwe_numpy as inp
    n = len(p.x)
    nb = (n + p.batch - 1) // p.batch
    tref = inp._to_sec(p.t_ref_ns)
    dt_b = np.array([inp._to_sec(inp.batch_time_ns(p.t_ns[b * p.batch], p.t_ns[min((b + 1) * p.batch, n) - 1])) - tref
                     for b in range(nb)])
    dt = dt_b[np.arange(n) // p.batch]
    b = p.lut[p.y.astype(np.int64) * p.W + p.x.astype(np.int64)]
    dr = np.asarray(omega, np.float64)[None, :] * dt[:, None]
    r = b + np.cross(dr, b)
    return p.fx * r[:, 0] / r[:, 2] + p.cx, p.fy * r[:, 1] / r[:, 2] + p.cy


def tiles_of(img):
    """boolean (tiles_y, tiles_x): 32 x 32 tiles of the image that hold a non-zero pixel"""
    ty, tx = (img.shape[0] + TILE - 1) // TILE, (img.shape[1] + TILE - 1) // TILE
    pad = np.zeros((ty * TILE, tx * TILE), bool)
    pad[:img.shape[0], :img.shape[1]] = np.asarray(img) != 0
    return pad.reshape(ty, TILE, tx, TILE).any(axis=(1, 3))


def moved_share(p, omega_sort, omega):
    """share of the events whose warped position at omega lies more than kBinMargin px from the one at omega_sort"""
    u0, v0 = positions(p, omega_sort)
    u1, v1 = positions(p, omega)
    return float(np.mean(np.maximum(np.abs(u1 - u0), np.abs(v1 - v0)) > BIN_MARGIN))


def fallback_share(p, omega_sort, omega, reach=0):
    """Model of stats()["fallback_frac"]: share of the events that vote at omega (inside the image) outside the LDS window --
    the 32 x 32 tile of their pixel at omega_sort and kBinMargin px on every side -- of the sort made at omega_sort.
    reach = kFuseReach: the share that votes further than that from the tile instead (what raises kFuseUnsafe)."""
    u0, v0 = positions(p, omega_sort)
    u1, v1 = positions(p, omega)
    x0, y0, x1, y1 = np.trunc(u0), np.trunc(v0), np.trunc(u1), np.trunc(v1)
    votes = (x1 >= 1) & (x1 < p.W - 2) & (y1 >= 1) & (y1 < p.H - 2)
    lx = x1 - (np.floor(x0 / TILE) * TILE - BIN_MARGIN)
    ly = y1 - (np.floor(y0 / TILE) * TILE - BIN_MARGIN)
    side = TILE + 2 * BIN_MARGIN
    if reach:
        lo, hi = BIN_MARGIN - reach, BIN_MARGIN + TILE - 1 + reach
        return float(np.mean(votes & ((lx < lo) | (lx + 1 > hi) | (ly < lo) | (ly + 1 > hi))))
    return float(np.mean(votes & ((lx < 0) | (lx >= side - 1) | (ly < 0) | (ly >= side - 1))))


def unreached_tiles(name, omega_sort, omega):
    """(row, col) of the tiles the oracle's unblurred IWE at omega votes into that lie more than kFuseNbr tiles, in either
    direction, from every tile occupied at omega_sort: inactive under the sort at omega_sort, out of every chunk's reach."""
    ref = fe_oracle(name)
    occ = tiles_of(ref.iwe(omega_sort, blur=False))
    now = tiles_of(ref.iwe(omega, blur=False))
    near = np.zeros_like(occ)
    for r, c in zip(*np.nonzero(occ)):
        near[max(r - FUSE_NBR, 0):r + FUSE_NBR + 1, max(c - FUSE_NBR, 0):c + FUSE_NBR + 1] = True
    return [(int(r), int(c)) for r, c in zip(*np.nonzero(now & ~near))]


def _far_candidates(omega_sort):
    for k in (12.0, 10.0, 14.0, 9.0, 16.0):
        for axis in (1, 0):
            for sgn in (1.0, -1.0):
                d = np.zeros(3)
                d[axis] = sgn * k
                yield np.asarray(omega_sort, np.float64) + d


def _far_point(name, omega_sort):
    p = packet(name)
    for om in _far_candidates(omega_sort):
        if moved_share(p, omega_sort, om) <= REBIN_FRAC and unreached_tiles(name, omega_sort, om):
            return om
    raise ValueError("no far point for packet %s at %s" % (name, omega_sort))


@functools.lru_cache(maxsize=None)
def _far_point_cached(name, key):
    return _far_point(name, np.array(key))


def far_point(name, omega_sort):
    """An omega, chosen from the oracle alone, at which (a) at most 3 % of the events of packet `name` lie more than 16 px from
    their position at omega_sort (no new sort) and (b) votes land in a tile out of the reach of every chunk of that sort."""
    return _far_point_cached(name, tuple(float(v) for v in omega_sort)).copy()


def reach_point(name, omega_sort):
    """Packet C: a step that carries both far groups out of their windows (fallback votes) but not beyond the reach."""
    return np.asarray(omega_sort, np.float64) + np.array([0.0, 4.0, 0.0])


def resort_point(name, omega_sort):
    """A jump after which more than 3 % of the votes of a sparse packet leave their windows, so that the evaluation after it
    sorts again.  The many events lie within 1 ms of the reference time: only a roll of hundreds of rad/s moves them by a
    window.  A rotation about the optical axis keeps the warp's denominator at 1 +- 0.03, so the point is as well-conditioned
    as any other; its gradient is small (the image is smeared), so the smallest roll that does it is taken."""
    p = packet(name)
    for k in (200.0, 250.0, 300.0, 350.0, 400.0, 450.0):
        for sgn in (1.0, -1.0):
            om = np.asarray(omega_sort, np.float64) + np.array([0.0, 0.0, sgn * k])
            if fallback_share(p, omega_sort, om) > REBIN_FRAC + 0.01:
                return om
    raise ValueError("no re-sort point for packet %s at %s" % (name, omega_sort))


# ------------------------------------------------------------------------------------------------- front-end walks
FE_OPTIONS = (("FUSED_IMAGE", (0, 1, 2, 3)), ("TAIL_FINALIZE", (0, 1, 4)), ("REUSE_IMAGE", (0, 1)), ("COMPOSITE_IMAGE", (0, 1)),
              ("CHAIN_SOLVE", (0, 1)))
FE_SEEDS = tuple(range(8))
FE_DET_SEEDS = (0, 1)
GRAD_FLOOR = 0.01   # every evaluation point's oracle gradient is at least this share of the largest over the list


FE_OPTION_LIST = tuple((k, v) for k, vs in FE_OPTIONS for v in vs)


class _FeGen:
    def __init__(self, seed, det=False):
        self.rng = np.random.default_rng(7000 + seed)
        self.det = det
        self.next_option = (5 * seed) % len(FE_OPTION_LIST)   # every seed walks the switches from another start: eight seeds cover them
        self.name = SPARSE[seed % 3]
        self.last = OMEGA0.copy()   # the point "near" steps start from
        self.prev = None            # index of the operation before this one if it evaluated ONE point (what "same" repeats)
        self.sort = OMEGA0.copy()   # where the generator believes the last sort was made (drives far_point only)
        self.resort = False         # ... and whether it believes the next evaluation sorts again, at its own point
        self.ops = []

    def near(self):
        return self.last + self.rng.normal(0, 0.3, 3)

    def point(self, kinds=("near", "near", "same", "far", "jump")):
        kind = str(self.rng.choice(kinds))
        if kind == "same" and self.prev is not None:
            return kind, self.ops[self.prev]["x"].copy()
        try:
            if kind == "far" and self.name in SPARSE:
                return kind, far_point(self.name, self.sort)
            if kind == "jump":
                return kind, (resort_point(self.name, self.sort) if self.name in SPARSE else self.sort + self.rng.choice([-1, 1], 3) * 6.0)
        except ValueError:   # (none from where the generator believes the sort to be)
            pass
        return "near", self.near()

    def moved_to(self, kind, x, grad=False):
        x = np.asarray(x, np.float64).copy()
        if self.resort:
            self.sort, self.resort = x, False
        if kind == "jump":
            self.resort = True   # the evaluation after the jump sorts at its own point
        if kind == "far" and grad:
            self.sort, self.resort = x, True   # (a fused evaluation beyond the reach repeats itself after a sort at its point)
        if kind == "near":
            self.last = x

    def step(self):
        rng = self.rng
        op = str(rng.choice(["eval", "eval", "eval", "eval_f", "eval_f", "hint_df", "eval_many", "eval_many", "eval_each", "iwe",
                             "iwe", "publish", "prepare", "set_packet", "solve", "option", "option", "option"]))
        prev, self.prev = self.prev, None
        if op in ("eval", "eval_f"):
            self.prev = prev
            kind, x = self.point()
            self.ops.append({"op": op, "x": x, "kind": kind})
            if kind == "same":
                self.ops[-1]["same_as"] = prev
            self.moved_to(kind, x, op == "eval")
            self.prev = len(self.ops) - 1
        elif op == "hint_df":
            _, x = self.point(("near",))
            self.ops.append({"op": op, "x": x, "kind": "near", "mode": int(rng.choice([1, 4])), "scale": float(rng.choice([0.5, 2.0]))})
            self.moved_to("near", x)
            self.prev = len(self.ops) - 1
        elif op in ("eval_many", "eval_each"):
            m = int(rng.integers(1, 5))
            xs, kinds = [], []
            for i in range(m):
                kind, x = self.point(("near", "far") if i == m - 1 else ("near", "near", "far"))
                xs.append(x)
                kinds.append(kind)
            self.ops.append({"op": op, "xs": np.array(xs), "kinds": kinds, "grad": bool(rng.integers(0, 2))})
        elif op == "iwe":
            kind, x = self.point(("near", "far"))
            self.ops.append({"op": op, "x": x, "kind": kind, "blur": bool(rng.integers(0, 2)),
                             "deriv": bool(rng.integers(0, 2)) and not self.det})   # (derivative planes: fp32 atomics, no promise of bits)
        elif op == "publish":
            kind, x = self.point(("near", "far"))
            self.ops.append({"op": op, "x": x, "kind": kind})
        elif op == "prepare":
            hint = self.near()
            self.ops.append({"op": op, "x": hint})
            self.sort, self.resort = hint.copy(), False
        elif op == "set_packet":
            self.name = str(rng.choice([n for n in PACKETS if n != self.name]))
            self.ops.append({"op": op, "packet": self.name})
            self.last = OMEGA0.copy()
            self.sort, self.resort = OMEGA0.copy(), False
            self.ops.append({"op": "eval", "x": OMEGA0.copy(), "kind": "near"})
            self.prev = len(self.ops) - 1
        elif op == "solve":
            far = bool(rng.integers(0, 2))
            self.ops.append({"op": op, "x": np.array([0.0, 14.0, 0.0]) if far else np.zeros(3), "far": far})
        else:
            key, value = FE_OPTION_LIST[self.next_option]
            self.next_option = (self.next_option + 1) % len(FE_OPTION_LIST)
            self.ops.append({"op": "option", "key": key, "value": value})
        for o in self.ops:
            o.setdefault("packet", self.name)


def _fe_eval_points(ops):
    """(op index, row or None) of every point an operation list asks a contrast or gradient at"""
    out = []
    for i, o in enumerate(ops):
        if o["op"] in ("eval", "eval_f", "hint_df"):
            out.append((i, None))
        elif o["op"] in ("eval_many", "eval_each"):
            out.extend((i, r) for r in range(len(o["xs"])))
    return out


def _fe_point(o, r):
    return o["x"] if r is None else o["xs"][r]


@functools.lru_cache(maxsize=None)
def fe_walk(seed, det=False):
    """The operation list of a seed (30 to 40 operations), every evaluation point with its oracle contrast and gradient
    ('c', 'g' / 'cs', 'gs').  A point whose gradient is under GRAD_FLOOR of the largest of the list is drawn again, near
    OMEGA0, from the seed's own stream -- here, never at comparison time.  det: a list for the deterministic mode (no
    read-back of derivative planes: they are voted with fp32 atomics, which that mode does not cover)."""
    g = _FeGen(seed, det)
    g.ops.append({"op": "eval", "x": OMEGA0.copy(), "kind": "near", "packet": g.name})
    g.prev = 0
    n_ops = 30 + int(g.rng.integers(0, 9))
    while len(g.ops) < n_ops:
        g.step()
    ops = g.ops[:40]
    pts = _fe_eval_points(ops)
    vals = {}
    redrawn = 0
    while True:
        for i, o in enumerate(ops):   # "same" follows the operation it repeats
            if "same_as" in o and not np.array_equal(o["x"], ops[o["same_as"]]["x"]):
                o["x"] = ops[o["same_as"]]["x"].copy()
                vals.pop((i, None), None)
        for i, r in pts:
            if (i, r) not in vals:
                vals[(i, r)] = fe_oracle(ops[i]["packet"]).eval(_fe_point(ops[i], r))
        top = max(np.abs(v[1]).max() for v in vals.values())
        low = sorted(k for k, v in vals.items() if np.abs(v[1]).max() < GRAD_FLOOR * top)
        if not low:
            break
        for i, r in low:
            del vals[(i, r)]
            if "same_as" in ops[i]:
                continue   # (what it repeats is as low and is drawn again: it follows)
            x = OMEGA0 + g.rng.normal(0, 0.3, 3)
            if r is None:
                ops[i]["x"], ops[i]["kind"] = x, "near"
            else:
                ops[i]["xs"][r], ops[i]["kinds"][r] = x, "near"
            ops[i]["redrawn"] = True
            redrawn += 1
        assert redrawn < 200, "the gradient-scale rule does not settle for seed %d" % seed
    for (i, r), (c, gr) in vals.items():
        o = ops[i]
        if r is None:
            o["c"], o["g"] = c, gr
        else:
            o.setdefault("cs", np.zeros(len(o["xs"])))[r] = c
            o.setdefault("gs", np.zeros((len(o["xs"]), 3)))[r] = gr
    return ops


def fe_alphabet(ops):
    """the set of alphabet letters an operation list uses (tests/test_seq_cases_cpu.py: every letter occurs in the seeds run)"""
    out = set()
    for o in ops:
        k = o["op"]
        if k in ("eval", "eval_f"):
            out.add("%s:%s" % (k, o["kind"]))
        elif k in ("eval_many", "eval_each"):
            out.add("%s:%s:%s" % (k, "grad" if o["grad"] else "cost", o["kinds"][-1]) if k == "eval_many" else k)
            if k == "eval_many":
                out.add("eval_many:len%d" % len(o["xs"]))
        elif k == "iwe":
            out.add("iwe:%s:%s" % ("blur" if o["blur"] else "raw", "deriv" if o["deriv"] else "plain"))
        elif k == "solve":
            out.add("solve:%s" % ("far" if o["far"] else "zero"))
        elif k == "option":
            out.add("option:%s=%d" % (o["key"], o["value"]))
        else:
            out.add(k)
    return out


FE_ALPHABET = (
    {"eval:near", "eval:same", "eval:far", "eval:jump", "eval_f:near", "eval_f:same", "eval_f:far", "eval_f:jump", "hint_df",
     "eval_each", "publish", "prepare", "set_packet", "solve:far", "solve:zero"}
    | {"eval_many:%s:%s" % (a, b) for a in ("grad", "cost") for b in ("near", "far")}
    | {"eval_many:len%d" % m for m in (1, 2, 3, 4)}
    | {"iwe:%s:%s" % (a, b) for a in ("blur", "raw") for b in ("deriv", "plain")}
    | {"option:%s=%d" % (k, v) for k, vs in FE_OPTIONS for v in vs})


def describe(ops, upto=None):
    """one line per operation, for assertion messages"""
    out = []
    for i, o in enumerate(ops if upto is None else ops[:upto + 1]):
        a = {k: (np.round(v, 4).tolist() if isinstance(v, np.ndarray) else v) for k, v in o.items()
             if k not in ("c", "g", "cs", "gs", "op", "window")}
        out.append("%2d %s %s" % (i, o["op"], a))
    return "\n".join(out)


# ------------------------------------------------------------------------------------------------- back end
BE_SEEDS = tuple(range(6))
BE_DET_SEEDS = (0, 1)


@functools.lru_cache(maxsize=None)
def be_window(which):
    """The sparse window recipe of tests/test_gpu_sparse_tiles.py on a 512 x 256 panorama: the camera sees a tenth of it."""
    n, seed = ((40_000, 71), (25_000, 73))[which]
    return synth.backend_window(n, W, H, FX, FY, CX, CY, 512, 256, 2, 5, 1, 0.2, seed=seed)


@functools.lru_cache(maxsize=None)
def be_map(which, kind):
    """None, a blob in a corner the camera never looks at ('far'), or that and one under the events ('both')"""
    if kind == "none":
        return None
    w = be_window(which)
    IG = np.zeros((w.Hp, w.Wp), np.float32)
    yy, xx = np.mgrid[0:w.Hp, 0:w.Wp]
    IG += (3.0 * np.exp(-((xx - 10) ** 2 + (yy - 250) ** 2) / 100.0)).astype(np.float32) * ((xx < 30) & (yy > 220))
    if kind == "both":
        IG += (2.0 * np.exp(-((xx - 260) ** 2 + (yy - 125) ** 2) / 450.0)).astype(np.float32) * (np.hypot(xx - 260, yy - 125) < 45)
    return IG


def be_oracle(which):
    w = be_window(which)
    return po.Backend(w.W, w.H, w.lut, w.Wp, w.Hp, w.order, w.batch, w.sample_rate, 1.0, po.VARIANCE)


def be_oracle_set_window(ref, which, kind):
    w = be_window(which)
    ref.set_window(w.x, w.y, w.t_ns, w.knots_init, w.start_ns, w.dt_ns, w.num_fixed, w.t_next_win_beg_ns, be_map(which, kind))


def _be_point(rng, P, last, big):
    kind = str(rng.choice(["near", "near", "same", "big", "jump"]))
    if kind == "same":
        return kind, last.copy()
    if kind == "big":      # a 14-degree yaw of every free knot: every vote lands ~20 px away, in other tiles; or back again
        return kind, (big if np.abs(last - big).max() > 0.1 else np.zeros(P)) + rng.normal(0, 0.002, P)
    if kind == "jump":
        return kind, rng.normal(0, 0.1, P)
    return kind, rng.normal(0, 0.01, P)


@functools.lru_cache(maxsize=None)
def be_walk(seed, det=False):
    """Operation list of a back-end seed, with the oracle's answers: the oracle object goes through the same set_window and
    evaluation sequence (its blend factor alpha belongs to the first evaluation after a set_window, as in the library).  Every
    evaluation point keeps the gradient-scale rule of the front-end walks: one that does not is drawn again here, at
    generation, never skipped at comparison time.  det: a list for the deterministic mode (every path switch chooses the production path: the
    reference-shaped one votes with fp32 atomics, which that mode does not cover)."""
    rng = np.random.default_rng(9000 + seed)
    which, kind = seed % 2, ("none", "far", "both")[seed % 3]
    P = be_window(which).P
    big = np.tile([0.0, 0.25, 0.0], P // 3)
    ops = [{"op": "set_window", "window": which, "map": kind}, {"op": "eval", "x": np.zeros(P), "kind": "near"}]
    last = np.zeros(P)
    n_ops = 30 + int(rng.integers(0, 9))
    while len(ops) < n_ops:
        op = str(rng.choice(["eval", "eval", "eval", "eval_f", "eval_f", "hint_df", "eval_many", "eval_each", "plane", "alpha",
                             "prepare", "set_window", "path"]))
        if op in ("eval", "eval_f", "hint_df"):
            k, x = _be_point(rng, P, last, big)
            o = {"op": op, "x": x, "kind": k}
            if op == "hint_df":
                o.update(mode=int(rng.choice([1, 4])), scale=float(rng.choice([0.5, 2.0])))
            ops.append(o)
            last = x
        elif op in ("eval_many", "eval_each"):
            xs = [_be_point(rng, P, last, big)[1] for _ in range(int(rng.integers(1, 5)))]
            ops.append({"op": op, "xs": np.array(xs), "grad": bool(rng.integers(0, 2))})
            last = xs[-1]
        elif op == "plane":
            ops.append({"op": op, "plane": str(rng.choice(["IL_old", "IL_new"]))})
        elif op == "alpha":
            ops.append({"op": op})
        elif op == "prepare":
            ops.append({"op": op, "x": None if rng.integers(0, 2) else rng.normal(0, 0.05, P)})
        elif op == "set_window":
            which, kind = int(rng.integers(0, 2)), str(rng.choice(["none", "far", "both"]))
            ops.append({"op": op, "window": which, "map": kind})
            ops.append({"op": "eval", "x": np.zeros(P), "kind": "near"})   # (both windows have the same P)
            last = np.zeros(P)
        else:
            ops.append({"op": "path", "fast": bool(rng.integers(0, 2)) or det})
    ops = ops[:40]
    # the oracle's answers, in call order; a point under the gradient floor is drawn again from the seed's stream (a small step,
    # like "near") and, the oracle being stateful in alpha and the planes, the whole list is answered again
    redrawn = 0
    while True:
        grads = _be_answers(ops)
        top = max(grads.values())
        low = sorted(k for k, v in grads.items() if v < GRAD_FLOOR * top)
        if not low:
            return ops
        for i, r in low:
            x = rng.normal(0, 0.01, P)
            if r is None:
                ops[i]["x"], ops[i]["kind"] = x, "near"
            else:
                ops[i]["xs"][r] = x
            ops[i]["redrawn"] = True
            redrawn += 1
        assert redrawn < 200, "the gradient-scale rule does not settle for back-end seed %d" % seed


def _be_answers(ops):
    """fills in the oracle's answers of a back-end list; returns {(op index, row or None): max-norm of the gradient there}"""
    grads, ref = {}, None
    for i, o in enumerate(ops):
        k = o["op"]
        if k == "set_window":
            ref = be_oracle(o["window"])
            be_oracle_set_window(ref, o["window"], o["map"])
        elif k in ("eval", "eval_f", "hint_df"):
            o["c"], o["g"] = ref.eval(o["x"], True)
            grads[(i, None)] = np.abs(o["g"]).max()
        elif k in ("eval_many", "eval_each"):
            r = [ref.eval(x, True) for x in o["xs"]]
            o["cs"], o["gs"] = np.array([v[0] for v in r]), np.array([v[1] for v in r])
            for j, v in enumerate(r):
                grads[(i, j)] = np.abs(v[1]).max()
        elif k == "plane":
            o["img"] = getattr(ref, o["plane"]).copy()
        elif k == "alpha":
            o["alpha"] = float(ref.alpha)
    return grads


def be_alphabet(ops):
    out = set()
    for o in ops:
        k = o["op"]
        if k in ("eval", "eval_f"):
            out.add("%s:%s" % (k, o["kind"]))
        elif k == "eval_many":
            out.add("eval_many:%s" % ("grad" if o["grad"] else "cost"))
        elif k == "set_window":
            out.add("set_window:%s" % ("map" if o["map"] != "none" else "nomap"))
        elif k == "path":
            out.add("path:%s" % ("fast" if o["fast"] else "reference"))
        elif k == "prepare":
            out.add("prepare:%s" % ("hint" if o["x"] is not None else "nohint"))
        else:
            out.add(k)
    return out


BE_ALPHABET = {"eval:near", "eval:same", "eval:big", "eval:jump", "eval_f:near", "eval_f:same", "eval_f:big", "eval_f:jump",
               "hint_df", "eval_many:grad", "eval_many:cost", "eval_each", "plane", "alpha", "prepare:hint", "prepare:nohint",
               "set_window:map", "set_window:nomap", "path:fast", "path:reference"}
