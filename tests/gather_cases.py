"""Inputs of the per-parameter gather tests (tests/test_gather_ref_cpu.py, tests/test_gpu_gather.py): event sets and splines chosen so
that every kind of gather error lands in a parameter of its own.  numpy, cmax_slam_amd.synth and the oracle only; built once per
process and shared, read-only.

Back end and whole trajectory -- "one batch per segment".  Events are evenly spaced in time inside their batch and the knot spacing
is one batch's duration, so batch b's pose time falls in knot segment seg(b) (= b unless the case has a gap; asserted here).  With
order 2 batch b then touches knots b and b + 1 only, with order 4 knots b .. b + 3: an event filed under the neighbouring batch shows
in a knot the right batch never reaches, and every knot sees a few batches' events, so one event is a large share of its entries.
Knots are a smooth random walk left-multiplied by exp(N(0, 0.05 rad)) per knot (recon_grad_cases.perturb): neighbouring batches'
Jacobians differ in the first digit, not the third.

per_batch runs over the lane structure of the gather kernels: 3, 63, 64, 65, 100, 128, 256 (one event per lane / four per lane, a
batch run below, at and above a wave), and the multiples of four on both sides of the fold rule (256 / per_batch + 2) 3 order <= 64:
84 | 88 at order 4, 28 | 32 at order 2.  n is never a multiple of 4, 64 or 256 (ragged last lane group), one case ends in a batch of
one event (which the reference never warps), one samples every third event.

Front end: all packets have fx = fy = 256 and integer cx, cy, so at omega = 0 the warp gives u = x exactly
(dense_image_ops.exact_packet's construction) and an event's place relative to the border is chosen by its pixel."""
import functools

import numpy as np

import dense_image_ops as dio
import gather_ref as gr
import recon_grad_cases as rg
from cmax_slam_amd import synth
from oracle import pyoracle as po

SENSOR = (240, 180, 200.0, 200.0, 119.5, 89.5)
PERTURB = 0.05
DT_EVENT_NS = 20_000  # spacing of the events in time; a batch of B events lasts B * DT_EVENT_NS = one knot interval


# ------------------------------------------------------------------------------------------------- back end / whole trajectory
def _be(order, per_batch, n, nf=0, rate=1, seed=1, Wp=256, Hp=128, gap=None, side=None, use_map=False, sigma=1.0, measure=0,
        seam=False):
    return dict(order=order, per_batch=per_batch, n=n, nf=nf, rate=rate, seed=seed, Wp=Wp, Hp=Hp, gap=gap, side=side, use_map=use_map,
                sigma=sigma, measure=measure, seam=seam)


def _ragged(per_batch, batches):
    """an event count with `batches` batches, the last one ragged, and no multiple of 4 (hence of 64 or 256)"""
    n = (batches - 1) * per_batch + max(2, (per_batch * 5) // 8)
    while n % 4 == 0 or n % per_batch == 1:
        n += 1
    assert (n - 1 + per_batch - 1) // per_batch == batches and n % 4
    return n


def _batches(per_batch):
    return int(np.clip(2400 // per_batch, 9, 60))  # a few thousand events at most, K <= 64 at order 4


# window path (K <= 64): name -> configuration
WINDOW = {}
for _o in (2, 4):
    for _pb in (3, 63, 64, 65, 100, 128, 256):
        WINDOW["o%d_b%d" % (_o, _pb)] = _be(_o, _pb, _ragged(_pb, _batches(_pb)), seed=10 * _pb + _o)
for _o, _pb in ((4, 84), (4, 88), (2, 28), (2, 32)):  # both sides of the fold rule
    WINDOW["o%d_b%d" % (_o, _pb)] = _be(_o, _pb, _ragged(_pb, _batches(_pb)), seed=10 * _pb + _o)
WINDOW["last_batch_of_one"] = _be(4, 64, 20 * 64 + 1, seed=3)                 # 20 batches and a single event nobody warps
WINDOW["rate3"] = _be(4, 200, _ragged(200, 12), rate=3, seed=4)               # 67 sampled events per batch, stride restarts
WINDOW["fixed1"] = _be(4, 88, _ragged(88, 27), nf=1, seed=5)                  # batch 0 loses its first knot's columns
WINDOW["fixed_mid"] = _be(4, 88, _ragged(88, 27), nf=14, seed=6)              # the line cuts batches 11 .. 13
WINDOW["fixed_mid_o2"] = _be(2, 100, _ragged(100, 24), nf=12, seed=7)         # ... and batch 11 at order 2 (unfolded kernels)
WINDOW["map"] = _be(4, 100, _ragged(100, 24), seed=8, use_map=True)           # alpha != 0
WINDOW["two_sides"] = _be(4, 100, _ragged(100, 24), seed=9, side=0.4)         # events on both sides of t_next_win_beg_ns
# the camera looks at the panorama's seam: votes in the border band of every batch, so every knot has a border sum S2 -- with 61
# free knots the S1 | S2 columns (366) outnumber the threads of the workgroup that finalizes (256)
WINDOW["seam_61_knots"] = _be(2, 28, _ragged(28, 60), seed=12, seam=True)
WINDOW["seam_o4"] = _be(4, 100, _ragged(100, 24), seed=13, seam=True, sigma=2.0)
WINDOW["sigma2_measure1"] = _be(2, 64, _ragged(64, 37), seed=11, sigma=2.0, measure=1)
PER_BATCH_CASES = [k for k in WINDOW if k.startswith("o")]
FORM_CASES = ["o4_b88", "o4_b84", "o2_b28", "o2_b63", "fixed_mid"]  # folded, unfolded four-per-lane, folded, one-per-lane, cut

# whole trajectory (any K)
RECON = {
    "long4": _be(4, 64, _ragged(64, 297), seed=21),                           # K = 300, cubic
    "long2": _be(2, 100, _ragged(100, 299), seed=22),                         # K = 300, linear
    "shared_batch": _be(4, 5000, 12_345, seed=23),                            # a batch of 5000 events walked by three workgroups
    "run_ends": _be(4, 100, 3 * 2048, seed=24),                               # n = 3 runs of recon_run(100) = 2048 events exactly
    "run_ends_b3": _be(2, 3, 2 * 768 + 2, seed=25),                           # recon_run(3) = 768: two full runs and one batch more
    "gap": _be(4, 64, _ragged(64, 24), seed=26, gap=(10, 270)),               # batches 10.. sit 270 knots on: outside the window
}


def _knots(K, seed, seam=False):
    rng = np.random.default_rng(seed)
    from scipy.spatial.transform import Rotation as Rot
    q, ks = Rot.identity(), []
    for _ in range(K):
        ks.append(q.as_quat())
        q = Rot.from_rotvec(rng.normal(0, 0.02, 3)) * q
    q = rg.perturb(np.array(ks), seed + 1, PERTURB)
    if seam:  # half a turn about y in front of every pose: the optical axis points at phi = +-pi
        q = rg._quat_mul(np.tile([0.0, 1.0, 0.0, 0.0], (K, 1)), q)
    return q


@functools.lru_cache(maxsize=None)
def be_case(kind, name):
    """(configuration, x, y, t_ns, lut, knots, start_ns, dt_ns, segments, IG or None, t_next_win_beg_ns)"""
    c = (WINDOW if kind == "window" else RECON)[name]
    W, H, fx, fy, cx, cy = SENSOR
    B, n = c["per_batch"], c["n"]
    rng = np.random.default_rng(c["seed"])
    nb = (n - 1 + B - 1) // B
    seg = np.arange(nb)
    if c["gap"]:
        seg[c["gap"][0]:] += c["gap"][1]
    K = int(seg[-1]) + c["order"]
    dt_ns = B * DT_EVENT_NS
    start_ns = synth.T0_NS
    i = np.arange(n)
    b = np.minimum(i // B, nb - 1)
    slot = i - b * B
    # (a trailing single event, which nobody warps, stays inside the spline's support: half a step behind the last batch's end)
    t = start_ns + seg[b] * dt_ns + np.minimum(slot, B - 1) * DT_EVENT_NS + np.where(slot >= B, DT_EVENT_NS // 2, DT_EVENT_NS // 4)
    # pixels: blobs of different weight over a uniform floor, so the panorama and Jt have structure at every scale
    nbl = 12
    bx, by = rng.uniform(20, W - 20, nbl), rng.uniform(20, H - 20, nbl)
    which = rng.integers(0, nbl, n)
    x = np.rint(bx[which] + 6.0 * rng.standard_normal(n))
    y = np.rint(by[which] + 6.0 * rng.standard_normal(n))
    floor = rng.random(n) < 0.4
    x[floor], y[floor] = rng.integers(0, W, int(floor.sum())), rng.integers(0, H, int(floor.sum()))
    x, y = np.clip(x, 0, W - 1).astype(np.uint16), np.clip(y, 0, H - 1).astype(np.uint16)
    knots = _knots(K, 100 + c["seed"], c["seam"])
    IG = rng.uniform(0.5, 2.0, (c["Hp"], c["Wp"])).astype(np.float32) if c["use_map"] else None
    side = 2 ** 62 if c["side"] is None else int(t[int(c["side"] * n)])
    for a in (x, y, t, knots):
        a.setflags(write=False)
    return c, x, y, t, synth.pinhole_lut(W, H, fx, fy, cx, cy), knots, start_ns, dt_ns, seg, IG, side


def be_point(kind, name):
    """the increments a window evaluation is made at (the whole-trajectory calls take knots, not increments)"""
    c, _, _, _, _, knots, *_ = be_case(kind, name)
    return 0.01 * np.cos(np.arange(3 * (len(knots) - c["nf"])))


@functools.lru_cache(maxsize=None)
def be_events(kind, name, nf=None):
    """the reference's EventList of a case at its evaluation point; nf overrides the case's num_fixed (frozen head)"""
    c, x, y, t, lut, knots, start_ns, dt_ns, seg, _, _ = be_case(kind, name)
    nf = c["nf"] if nf is None else nf
    k = po.left_update(knots, be_point(kind, name), c["nf"]) if kind == "window" else knots
    ev = gr.be_events(x, y, t, lut, SENSOR[0], c["Wp"], c["Hp"], c["order"], k, start_ns, dt_ns, nf, c["per_batch"], c["rate"])
    check_layout(ev, seg)
    return ev


def check_layout(ev, seg):
    """what the construction promises, on the CPU: batch b's pose time lies in segment seg(b), no panorama coordinate within
    CELL_MARGIN of an integer, and events vote"""
    assert np.array_equal(ev.info["segment"], seg[:len(ev.info["segment"])]), "a batch's pose time left its segment"
    assert ev.margin > gr.CELL_MARGIN, "a panorama coordinate lies %.2e px from an integer: change the seed" % ev.margin
    assert ev.n > 0


# ------------------------------------------------------------------------------------------------------------------ front end
FE_W, FE_H = 100, 70
FE_OMEGAS = ((0.0, 0.0, 0.0), (0.4, -0.6, 0.9))
FE_COUNTS = (1, 255, 256, 257, 1023, 1025, 65_537, 131_000)


def _packet(W, H, x, y, rng):
    n = len(x)
    T = 0.05
    t_ns = synth.T0_NS + np.sort(np.floor(rng.random(n) * T * 1e9).astype(np.int64))
    p = synth.FrontendPacket(W, H, 256.0, 256.0, float(W // 2), float(H // 2), np.asarray(x, np.uint16), np.asarray(y, np.uint16), t_ns,
                             synth.T0_NS + int(round(T / 2 * 1e9)), np.zeros(3))
    for a in (p.x, p.y, p.t_ns):
        a.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def fe_packet(kind, sigma=1.0, n=None):
    """kind: 'exact' dense_image_ops.exact_packet; 'band' every event within the border band of width r (at omega = 0); 'corners'
    every event in the four r x r corners; 'last' every event on the last accepted cells xx = 1, xx = W - 3, yy = 1, yy = H - 3;
    'count' n events on uniformly random pixels of a 240 x 180 sensor."""
    r = max(dio.radius(sigma), 1)
    if kind == "exact":
        return dio.exact_packet(FE_W, FE_H)
    if kind == "count":
        rng = np.random.default_rng(7000 + n)
        W, H = 240, 180
        return _packet(W, H, rng.integers(1, W - 2, n), rng.integers(1, H - 2, n), rng)
    W, H = FE_W, FE_H
    rng = np.random.default_rng({"band": 71, "corners": 72, "last": 73}[kind] + int(10 * sigma))
    lo_x, hi_x = np.arange(1, r + 1), np.arange(W - 2 - r, W - 2)   # xx <= r | xx + 1 >= W - 1 - r, inside the accepted cells
    lo_y, hi_y = np.arange(1, r + 1), np.arange(H - 2 - r, H - 2)
    m = 3000
    if kind == "corners":
        x, y = rng.choice(np.concatenate([lo_x, hi_x]), m), rng.choice(np.concatenate([lo_y, hi_y]), m)
    elif kind == "band":
        x, y = rng.integers(1, W - 2, m), rng.integers(1, H - 2, m)
        on_x = rng.random(m) < 0.5
        x[on_x] = rng.choice(np.concatenate([lo_x, hi_x]), int(on_x.sum()))
        y[~on_x] = rng.choice(np.concatenate([lo_y, hi_y]), int((~on_x).sum()))
    else:
        x, y = rng.integers(1, W - 2, m), rng.integers(1, H - 2, m)
        q = rng.integers(0, 4, m)
        x[q == 0], x[q == 1], y[q == 2], y[q == 3] = 1, W - 3, 1, H - 3
    # uneven weights: a quarter of the events repeat a few pixels, so Jt has slopes in the band and not a plateau
    heavy = rng.random(m) < 0.25
    pick = rng.integers(0, 8, int(heavy.sum()))
    x[heavy], y[heavy] = x[:8][pick], y[:8][pick]
    return _packet(W, H, x, y, rng)


def fe_events(p, omega):
    return gr.fe_events(p, omega)
