"""Probe packets of the per-event front-end vote tests (tests/test_fe_probe_cases_cpu.py, tests/test_gpu_fe_votes.py): numpy,
cmax_slam_amd.synth and the numpy oracle only; built once per process and shared, read-only.

A probe packet keeps the 2 x 2 vote cell of every voting event disjoint from every other event's and a ring of one empty pixel
around it, at EVERY angular velocity of the case's list at once: at each of them the forward plane IS the list of votes, one event
per cell, and a wrong dt, bearing, weight, accept rule or a stale vote is an error of the order of a vote in one cell, with nothing
to average it away.

Construction, batch by batch.  A front-end dt belongs to the batch (the middle of its first and last timestamp,
oracle.iwe_numpy.batch_time_ns), so selecting events from a finished packet would change the warp of all the others.  Batch b
therefore has a fixed first and last timestamp (hence a fixed dt_b) before any of its events exists; random sensor pixels are
warped with dt_b at every omega of the list (gather_ref.fe_events' arithmetic = fe_warp_math operation for operation), and a
candidate joins the batch only if, at every omega at which it votes, its cell and ring are free in that omega's occupancy map --
until the batch holds exactly `batch` events (the last batch is ragged).  Interior timestamps are sorted random values between the
two fixed ends.  A candidate whose u or v lies within INT_MARGIN of an integer at a non-zero omega is rejected (the fp64 reference
weights then do not depend on the last bits of u).  fx = fy = 256 and integer cx, cy (dense_image_ops.exact_packet's LUT): at
omega = 0 the warp gives u = x exactly -- asserted; case unit_lut normalises the LUT's rows to unit length (the z column is not all
ones: no two-column bearing table, the kernels that load bearings per event) and is exempt from that assertion.  Non-finite and
out-of-range u, v are decided before any integer cast (gather_ref.device_int).

Host model of the tile sort (predicted_fallback / predicted_unsafe): cmx_binning.hip's tile_key, build_chunks_kernel's window
origin and fe_splat_lds_body's window and reach conditions, in integers."""
import functools
from dataclasses import dataclass

import numpy as np

import gather_ref as gr
from cmax_slam_amd import synth
from oracle import iwe_numpy as inp

TILE, MARGIN, REACH = 32, 16, 56          # kBinTile, kBinMargin, kFuseReach (cmx_internal.hpp)
WINDOW = TILE + 2 * MARGIN                # kBinWindow
# per cell: three fp32 roundings of values <= 1 on the way to a weight (the cast of dx, 1 - dx, the product; a factor pair has at
# most 2.5 * 2^-24 in all), one 2^-30 fixed-point unit and the cast back on the LDS and deterministic forms
BOUND = 4 * 2.0 ** -24 + 2.0 ** -30
INT_MARGIN = 1e-6
CATCH = 100.0                             # a mutation must exceed BOUND this many times over at some cell

W0 = (0.0, 0.0, 0.0)
W1 = (0.4, -0.6, 0.9)
W2 = (0.45, -0.55, 0.95)                  # W1 + 0.05 on every axis: a line search's step, no vote leaves its window
W3 = (6.0, -5.0, 9.0)                     # tests/test_gpu_fused.py's jump: votes leave their windows
OMEGAS = (W0, W1, W2, W3)
FAR_OMEGA = (60.0, -70.0, 20.0)           # most events leave the image, rz reaches zero and below

T_PACKET = 0.05
T_REF_OFFSET_NS = 25_137_911          # near the packet's middle, on no batch's own time: no batch has dt = 0 (u = x at every omega)


@dataclass(frozen=True)
class Case:
    W: int
    H: int
    batch: int
    n: int
    omegas: tuple = OMEGAS
    unit_lut: bool = False
    seed: int = 1
    region: tuple = None      # (x0, y0, x1, y1): sensor pixels are drawn from this rectangle only


CASES = {
    "one_tile_row": Case(100, 70, 100, 537, seed=11),      # partial tiles on both axes, one sort slice
    "tiny": Case(33, 35, 16, 37, seed=12),                 # two sort tiles per axis, the far ones 1 / 3 px wide
    "qvga": Case(240, 180, 100, 2937, seed=13),            # last batch of 37
    "qvga_b257": Case(240, 180, 257, 11 * 257 + 3, seed=14),   # last batch of 3; runs straddle waves and the 512-thread stride
    "two_slices": Case(640, 480, 100, 8237, seed=15),      # > 2 x 4096 events: three sort slices
    "unit_lut": Case(240, 180, 100, 2937, unit_lut=True, seed=13),
    "far": Case(240, 180, 100, 2937, omegas=(FAR_OMEGA,), seed=16),
    # events in one corner of the sensor: most sort tiles hold no vote, so a fused evaluation's tile passes clear the ping-pong
    # partner under the active tiles only, and W3 moves the votes onto other tiles than W0 .. W2 use
    "sparse": Case(240, 180, 100, 437, seed=17, region=(150, 100, 240, 180)),
}
COVERAGE_CASES = [k for k in CASES if k not in ("tiny", "far", "sparse")]


@dataclass
class ProbePacket:
    """what FrontendEvaluator.set_packet and gather_ref.fe_events read, with the LUT as a field"""
    W: int
    H: int
    fx: float
    fy: float
    cx: float
    cy: float
    x: np.ndarray
    y: np.ndarray
    t_ns: np.ndarray
    t_ref_ns: int
    lut: np.ndarray
    batch: int
    sigma: float = 1.0


def warp_uv(b, dt, omega, fx, fy, cx, cy):
    """(u, v) of bearings b (n x 3) at dt (n) -- the lines of gather_ref.fe_events"""
    wx, wy, wz = (float(w) for w in omega)
    px, py, pz = b[:, 0], b[:, 1], b[:, 2]
    drx, dry, drz = wx * dt, wy * dt, wz * dt
    rx = px + (dry * pz - drz * py)
    ry = py + (drz * px - drx * pz)
    rz = pz + (drx * py - dry * px)
    with np.errstate(all="ignore"):
        iz = 1.0 / rz
        cxn, cyn = rx * iz, ry * iz
        return fx * cxn + cx, fy * cyn + cy


def accepted(xx, yy, W, H):
    return (1 <= xx) & (xx < W - 2) & (1 <= yy) & (yy < H - 2)


def batch_dts(t_ns, t_ref_ns, batch):
    n = len(t_ns)
    nb = (n + batch - 1) // batch
    tref = inp._to_sec(t_ref_ns)
    return np.array([inp._to_sec(inp.batch_time_ns(t_ns[b * batch], t_ns[min((b + 1) * batch, n) - 1])) - tref for b in range(nb)])


def _lut(c):
    lut = synth.pinhole_lut(c.W, c.H, 256.0, 256.0, float(c.W // 2), float(c.H // 2))
    if c.unit_lut:
        lut = lut / np.sqrt((lut * lut).sum(axis=1, keepdims=True))
    return np.ascontiguousarray(lut)


def _candidates(rng, m, W, H, region=None):
    """uniform sensor pixels; a fifth of them on the three outermost columns / rows of either side and the one behind them, so
    that the last accepted cells (xx = 1, W - 3, yy = 1, H - 3) and the pixels that do not vote at omega = 0 are well filled"""
    if region is not None:
        return rng.integers(region[0], region[2], m), rng.integers(region[1], region[3], m)
    x, y = rng.integers(0, W, m), rng.integers(0, H, m)
    band_x = np.concatenate([np.arange(0, 4), np.arange(W - 4, W)])
    band_y = np.concatenate([np.arange(0, 4), np.arange(H - 4, H)])
    kind = rng.random(m)
    bx, by = kind < 0.1, (kind >= 0.1) & (kind < 0.2)
    x[bx] = rng.choice(band_x, int(bx.sum()))
    y[by] = rng.choice(band_y, int(by.sum()))
    return x, y


@functools.lru_cache(maxsize=None)
def packet(name):
    c = CASES[name]
    W, H = c.W, c.H
    rng = np.random.default_rng(c.seed)
    fx = fy = 256.0
    cx, cy = float(W // 2), float(H // 2)
    lut = _lut(c)
    nb = (c.n + c.batch - 1) // c.batch
    t_ref = synth.T0_NS + T_REF_OFFSET_NS
    occ = np.zeros((len(c.omegas), H, W), bool)
    xs, ys, ts = [], [], []
    for b in range(nb):
        size = min(c.batch, c.n - b * c.batch)
        t_first = synth.T0_NS + int(b * T_PACKET * 1e9) // nb
        t_last = synth.T0_NS + int((b + 1) * T_PACKET * 1e9) // nb - 1
        dt_b = inp._to_sec(inp.batch_time_ns(t_first, t_last)) - inp._to_sec(t_ref)
        bx, by = [], []
        rounds = 0
        while len(bx) < size:
            rounds += 1
            assert rounds < 400, "%s: batch %d cannot be filled: the image is full" % (name, b)
            m = 4 * size
            x, y = _candidates(rng, m, W, H, c.region)
            rows = lut[y * W + x]
            good = np.ones(m, bool)
            cells = []
            for k, om in enumerate(c.omegas):
                u, v = warp_uv(rows, np.full(m, dt_b), om, fx, fy, cx, cy)
                xx, yy = gr.device_int(u), gr.device_int(v)
                if any(om):
                    fin = np.isfinite(u) & np.isfinite(v)
                    near = np.zeros(m, bool)
                    near[fin] = (np.abs(u[fin] - np.rint(u[fin])) < INT_MARGIN) | (np.abs(v[fin] - np.rint(v[fin])) < INT_MARGIN)
                    good &= ~near
                elif not c.unit_lut:
                    assert np.array_equal(u, x.astype(np.float64)) and np.array_equal(v, y.astype(np.float64))
                cells.append((xx, yy, accepted(xx, yy, W, H)))
            for i in np.flatnonzero(good):
                free = all(not ok[i] or not occ[k, yy[i] - 1:yy[i] + 3, xx[i] - 1:xx[i] + 3].any()
                           for k, (xx, yy, ok) in enumerate(cells))
                if not free:
                    continue
                for k, (xx, yy, ok) in enumerate(cells):
                    if ok[i]:
                        occ[k, yy[i]:yy[i] + 2, xx[i]:xx[i] + 2] = True
                bx.append(x[i])
                by.append(y[i])
                if len(bx) == size:
                    break
        inner = np.sort(rng.integers(t_first, t_last + 1, max(size - 2, 0)))
        assert size > 1
        t = np.concatenate([[t_first], inner, [t_last]])
        xs.append(np.array(bx))
        ys.append(np.array(by))
        ts.append(t.astype(np.int64))
    p = ProbePacket(W, H, fx, fy, cx, cy, np.concatenate(xs).astype(np.uint16), np.concatenate(ys).astype(np.uint16),
                    np.concatenate(ts), t_ref, lut.reshape(-1), c.batch)
    assert len(p.x) == c.n and np.all(np.diff(p.t_ns) >= 0)
    for a in (p.x, p.y, p.t_ns, p.lut):
        a.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def events(name, omega):
    """gather_ref.fe_events of the case's packet at omega (a tuple), shared and read-only"""
    return gr.fe_events(packet(name), omega)


@functools.lru_cache(maxsize=None)
def reference(name, omega):
    """(fp64 plane of the votes, mask of the voting cells)"""
    ev = events(name, omega)
    ref = gr.forward_plane(ev, exact=True)
    mask = np.zeros((ev.H, ev.W), bool)
    for oy in (0, 1):
        for ox in (0, 1):
            mask[ev.yy + oy, ev.xx + ox] = True
    ref.setflags(write=False)
    mask.setflags(write=False)
    return ref, mask


# ---------------------------------------------------------------------------------------------------------------- comparison
def cell_errors(plane, name, omega):
    """(worst |plane - reference| over BOUND inside the voting cells, its pixel, the number of non-zero pixels outside them)"""
    ref, mask = reference(name, tuple(omega))
    plane = np.asarray(plane)
    assert plane.shape == ref.shape, (plane.shape, ref.shape)
    err = np.where(mask, np.abs(plane.astype(np.float64) - ref), 0.0)
    err[~np.isfinite(err)] = np.inf
    at = np.unravel_index(int(np.argmax(err)), err.shape) if err.size else (0, 0)
    return float(err[at]) / BOUND if mask.any() else 0.0, (int(at[0]), int(at[1])), int(np.count_nonzero(plane[~mask]))


def compare(tag, plane, name, omega):
    """the comparison of the GPU test: every voting cell within BOUND of the fp64 vote, every other pixel exactly 0, the plane's
    sum the number of voting events.  Returns the worst cell's error over BOUND."""
    ev = events(name, tuple(omega))
    ratio, at, outside = cell_errors(plane, name, omega)
    assert np.isfinite(np.asarray(plane)).all(), "%s: the plane is not finite" % tag
    assert outside == 0, "%s: %d pixels outside the voting cells are not zero" % (tag, outside)
    assert ratio <= 1.0, "%s: %s" % (tag, describe(plane, name, omega, at))
    total = float(np.asarray(plane).sum(dtype=np.float64))
    assert abs(total - ev.n) <= 4 * BOUND * max(ev.n, 1), "%s: the plane sums to %.9g, %d events vote" % (tag, total, ev.n)
    return ratio


def describe(plane, name, omega, at):
    ev, (ref, _) = events(name, tuple(omega)), reference(name, tuple(omega))
    y, x = at
    e = np.flatnonzero((ev.yy <= y) & (y <= ev.yy + 1) & (ev.xx <= x) & (x <= ev.xx + 1))
    who = "no event"
    if len(e):
        i = int(e[0])
        p = packet(name)
        who = "event %d (batch %d, sensor pixel %d, %d; cell %d, %d; dx %.9g dy %.9g)" % (
            ev.src[i], ev.src[i] // p.batch, p.x[ev.src[i]], p.y[ev.src[i]], ev.xx[i], ev.yy[i], ev.dx64[i], ev.dy64[i])
    return "pixel (x %d, y %d): plane %.9g, reference %.9g, |difference| %.3e = %.1f bounds; %s" % (
        x, y, float(np.asarray(plane)[y, x]), ref[y, x], abs(float(np.asarray(plane)[y, x]) - ref[y, x]),
        abs(float(np.asarray(plane)[y, x]) - ref[y, x]) / BOUND, who)


def derivative_reference(name, omega):
    """(3, n, 4): per voting event and corner, the signed fp64 weights times J64 -- fe_splat_kernel<true>'s four expressions"""
    ev = events(name, tuple(omega))
    dx, dy = ev.dx64, ev.dy64
    out = np.empty((3, ev.n, 4))
    for k in range(3):
        r0, r1 = ev.J64[:, 0, k], ev.J64[:, 1, k]
        out[k] = np.stack([r0 * (-(1 - dy)) + r1 * (-(1 - dx)), r0 * (1 - dy) + r1 * (-dx), r0 * (-dy) + r1 * (1 - dx), r0 * dy + r1 * dx],
                          axis=1)
    return out


# ------------------------------------------------------------------------------------------------------- the sort's host model
def _all_cells(name, omega):
    """(xx, yy, ok) of EVERY event at omega, with the device's integer conversion"""
    p = packet(name)
    x, y = p.x.astype(np.int64), p.y.astype(np.int64)
    dt = batch_dts(p.t_ns, p.t_ref_ns, p.batch)[np.arange(len(x)) // p.batch]
    u, v = warp_uv(p.lut.reshape(-1, 3)[y * p.W + x], dt, omega, p.fx, p.fy, p.cx, p.cy)
    xx, yy = gr.device_int(u), gr.device_int(v)
    return xx, yy, accepted(xx, yy, p.W, p.H), u, v


def sort_keys(name, omega_sort):
    """(tile x, tile y, has a window) per event: tile_key's rule"""
    p = packet(name)
    xx, yy, ok, _, _ = _all_cells(name, omega_sort)
    beyond = ~ok & ((xx < 1 - MARGIN) | (xx >= p.W - 2 + MARGIN) | (yy < 1 - MARGIN) | (yy >= p.H - 2 + MARGIN))
    cx_, cy_ = np.clip(xx, 1, p.W - 3), np.clip(yy, 1, p.H - 3)
    return cx_ // TILE, cy_ // TILE, ~beyond


def _outside(name, omega_sort, omega_eval):
    tx, ty, has_win = sort_keys(name, tuple(omega_sort))
    xx, yy, ok, _, _ = _all_cells(name, tuple(omega_eval))
    lx, ly = xx - (tx * TILE - MARGIN), yy - (ty * TILE - MARGIN)
    inside = has_win & (0 <= lx) & (lx < WINDOW - 1) & (0 <= ly) & (ly < WINDOW - 1)
    lo, hi = MARGIN - REACH, MARGIN + TILE - 1 + REACH
    far = ~has_win | (lx < lo) | (lx + 1 > hi) | (ly < lo) | (ly + 1 > hi)
    return ok & ~inside, ok & ~inside & far


def predicted_fallback(name, omega_sort, omega_eval):
    """the number of voting events at omega_eval that leave the LDS window of the tile they were sorted into at omega_sort"""
    return int(_outside(name, omega_sort, omega_eval)[0].sum())


def predicted_unsafe(name, omega_sort, omega_eval):
    """whether one of them lands beyond the reach the fused tiles' arrival counts cover (or has no window at all): the fused forms
    then repeat the evaluation behind a fresh sort"""
    return bool(_outside(name, omega_sort, omega_eval)[1].any())


def sort_slices(n):
    """bin_grid (cmx_binning.hip): the number of slices the counting sort walks"""
    blocks = min(max((n + 4095) // 4096, 1), 512)
    per_block = ((n + blocks - 1) // blocks + 1023) // 1024 * 1024
    return (n + per_block - 1) // per_block


# ---------------------------------------------------------------------------------------------------------------- mutations
def plane_of(u, v, W, H, keep=None, permute=None):
    """the fp64 plane of the events at (u, v); keep: a mask applied on top of the accept rule; permute: (event, order of its four
    weights)"""
    xx, yy = gr.device_int(u), gr.device_int(v)
    ok = accepted(xx, yy, W, H)
    if keep is not None:
        ok = ok & keep
    xx, yy, dx, dy = xx[ok], yy[ok], (u - xx)[ok], (v - yy)[ok]
    w = np.stack([(1 - dx) * (1 - dy), dx * (1 - dy), (1 - dx) * dy, dx * dy], axis=1)
    if permute is not None:
        e, order = permute
        j = int(np.flatnonzero(np.flatnonzero(ok) == e)[0])
        w[j] = w[j][list(order)]
    img = np.zeros((H, W))
    for k, (oy, ox) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
        np.add.at(img, (yy + oy, xx + ox), w[:, k])
    return img


def mutated_planes(name, omega, omega_prev):
    """{mutation: fp64 plane}: the five ways a splat can be subtly wrong, each applied to the reference's own arithmetic"""
    p = packet(name)
    W, H, n = p.W, p.H, len(p.x)
    x, y = p.x.astype(np.int64), p.y.astype(np.int64)
    rows = p.lut.reshape(-1, 3)[y * W + x]
    dts = batch_dts(p.t_ns, p.t_ref_ns, p.batch)
    b = np.arange(n) // p.batch
    args = (p.fx, p.fy, p.cx, p.cy)
    u, v = warp_uv(rows, dts[b], omega, *args)
    xx, yy = gr.device_int(u), gr.device_int(v)
    ok = accepted(xx, yy, W, H)
    out = {}
    # 1. every event warped with the next batch's dt (the last batch keeps its own)
    out["next_batch_dt"] = plane_of(*warp_uv(rows, dts[np.minimum(b + 1, len(dts) - 1)], omega, *args), W, H)
    # ... and only the LAST event of one batch (a run end of the sorted dt stream off by one)
    ends = np.arange(1, len(dts)) * p.batch - 1
    ends = ends[ok[ends]]
    assert len(ends), "%s: no batch ends in a voting event" % name
    last = int(ends[len(ends) // 2])
    dt1 = dts[b].copy()
    dt1[last] = dts[b[last] + 1]
    out["one_event_next_batch_dt"] = plane_of(*warp_uv(rows, dt1, omega, *args), W, H)
    # 2. one event warped with another event's bearing from the same sort tile (two sorted positions exchanged in one stream)
    tile = (yy // TILE) * 1000 + xx // TILE
    e = e2 = None
    for cand in np.flatnonzero(ok):
        other = np.flatnonzero(ok & (tile == tile[cand]) & ((x != x[cand]) | (y != y[cand])))
        if len(other):
            e, e2 = int(cand), int(other[0])
            break
    assert e is not None, "%s: no sort tile holds two voting events" % name
    rows2 = rows.copy()
    rows2[e] = rows[e2]
    out["swapped_bearing"] = plane_of(*warp_uv(rows2, dts[b], omega, *args), W, H)
    # 3. the events of the last accepted column rejected
    assert (ok & (xx == W - 3)).any(), "%s: no voting event on xx = W - 3" % name
    out["last_column_rejected"] = plane_of(u, v, W, H, keep=xx != W - 3)
    # 4. the four weights of one event permuted (the event whose weights differ most)
    dx, dy = u - xx, v - yy
    spread = np.where(ok, np.abs(dx - 0.5) * np.abs(dy - 0.5), -1.0)
    out["permuted_weights"] = plane_of(u, v, W, H, permute=(int(np.argmax(spread)), (1, 2, 3, 0)))
    # 5. one vote of the previous omega left in the plane
    up, vp = warp_uv(rows, dts[b], omega_prev, *args)
    xp, yp = gr.device_int(up), gr.device_int(vp)
    one = np.zeros(n, bool)
    one[int(np.flatnonzero(accepted(xp, yp, W, H))[0])] = True
    out["stale_vote"] = plane_of(u, v, W, H) + plane_of(up, vp, W, H, keep=one)
    return out


def displacement(name, omega_a, omega_b):
    """per event, the distance in pixels between its warps at the two omegas (events finite at both)"""
    _, _, _, ua, va = _all_cells(name, tuple(omega_a))
    _, _, _, ub, vb = _all_cells(name, tuple(omega_b))
    fin = np.isfinite(ua) & np.isfinite(va) & np.isfinite(ub) & np.isfinite(vb)
    return np.hypot(ua[fin] - ub[fin], va[fin] - vb[fin])
