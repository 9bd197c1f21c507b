"""Inputs for the back-end warp tests away from the panorama's centre (tests/test_far_cases_cpu.py checks them without a
GPU, tests/test_gpu_far_orientations.py runs them).  numpy + scipy only: nothing here touches a device.

(a) Probe tables: a bearing table for a 64 x 64 sensor, one event per sensor pixel (x = i % 64, y = i // 64), in which every
    pixel's bearing is chosen so that under the camera orientation Q its vote lands on a prescribed panorama position, and the
    2 x 2 cells of any two votes are disjoint.  A plane of such votes can be read back event by event: one cell off, or a border
    rule off by one, is a whole cell's worth of difference and not 1/N-th of a contrast.
    The panorama is cut into 4 x 4 slots and a probe owns one slot: target = 4 * slot + o + frac with o in {0, 1}, so columns /
    rows 4 s .. 4 s + 2 are touched at most and the next slot's stay free; in the LAST slot column / row o is in {0 .. 3}, so that
    targets reach Wp-4 .. Wp-1 and Hp-4 .. Hp-1 (those on Wp-2, Wp-1, Hp-2, Hp-1 are dropped by the border rule, as are those on
    column / row 0).  A quarter of the probes -- or every border slot, where the panorama has fewer than that: 380 at 512 x 256,
    646 at 1000 x 300 -- sit in the first / last slot row / column (both sides of the +-pi seam, both poles); the others in
    random interior slots.  frac is uniform in [0.02, 0.98], and 1e-6, 1 - 1e-6 or 0.5 for about a tenth of the probes.
    Bearing = Q^-1 * ray(target) times a random scale in [0.5, 3]: a general three-column table, z of either sign, |b| != 1.
    z1=True: slots only where the ray lies within 75 degrees of Q's optical axis, stored as b / b_z with z = 1 (the two-column
    16-byte load and the Z1 rotation).  That cone reaches a border only where the camera looks at one: none at the identity, one
    pole row and the seam next to it at a pitch of 90 degrees.
    The last two probes are the poles themselves, bearing = Q^-1 * (0, +-1, 0) exactly: atan2(0, 0), pixel row 0 or Hp.  (z1:
    only a pole in front of the camera can be written with z = 1; where none is, these two are ordinary probes.)
    One event per sensor pixel, fewer only where a z = 1 cone holds fewer slots than the sensor has pixels (512 x 256).
    All timestamps are equal and both knots of the (linear, K = 2) spline are Q, so every batch pose is Q.
(b) probe_reference: the forward projection of the table AS STORED under a given R, in np.longdouble.
(c) Far windows: synth's windows with the whole trajectory turned by Q (the events stay: e_ray_w = R * e_ray_cam, so the scene
    turns with the camera) -- at the seam, at the poles and behind the panorama's centre."""
import dataclasses
import functools

import numpy as np
from scipy.spatial.transform import Rotation as Rot

from cmax_slam_amd import synth

SENSOR = 64                       # the probe sensor is SENSOR x SENSOR, one event per pixel
N_PROBES = SENSOR * SENSOR
BATCH = 100                       # N_PROBES % BATCH = 96: no trailing one-event batch (the reference skips such a batch)
MIN_DIST = 1e-7                   # every probe but the poles keeps this distance from an integer pixel coordinate
PANOS = [(512, 256), (1000, 300)]
DT_NS = 50_000_000
T_EVENT_NS = synth.T0_NS + DT_NS // 2
LD = np.longdouble

PROBE_ORIENTATIONS = {
    "identity": Rot.identity(),
    "yaw180": Rot.from_euler("y", 180, degrees=True),
    "pitch90": Rot.from_euler("x", 90, degrees=True),
    "general": Rot.from_rotvec([1.3, -2.1, 0.7]),
}
# (orientation, z1) of every table the GPU test uses
PROBE_CASES = [("identity", False), ("yaw180", False), ("pitch90", False), ("general", False), ("identity", True), ("pitch90", True)]


def focal(Wp, Hp):
    """fx, fy of the equirectangular camera: focalFromFOV(size, 360 | 180) as be_args (cmx_pipeline.cpp) writes it"""
    return (Wp / 360.0) * 180.0 / 3.1415926535897932384626433832795, (Hp / 180.0) * 180.0 / 3.1415926535897932384626433832795


def _ray(px, py, Wp, Hp):
    fx, fy = focal(Wp, Hp)
    phi, th = (px - Wp / 2.0) / fx, (py - Hp / 2.0) / fy
    return np.stack([np.cos(th) * np.sin(phi), np.sin(th), np.cos(th) * np.cos(phi)], -1)


@dataclasses.dataclass
class ProbeTable:
    Wp: int
    Hp: int
    Q: Rot
    z1: bool
    lut: np.ndarray        # N_PROBES x 3 bearings, index y * SENSOR + x (rows n .. : (0, 0, 1), no event reads them)
    target: np.ndarray     # n x 2 intended pixel coordinate (px, py); the poles: nan
    n_pole: int            # the last n_pole probes are the poles
    n: int                 # events = probes: sensor pixels 0 .. n-1 (N_PROBES wherever the panorama has the slots)

    @property
    def bearings(self):
        return self.lut[:self.n]

    @property
    def x(self):
        return (np.arange(self.n) % SENSOR).astype(np.uint16)

    @property
    def y(self):
        return (np.arange(self.n) // SENSOR).astype(np.uint16)

    @property
    def t_ns(self):
        return np.full(self.n, T_EVENT_NS, np.int64)

    @property
    def knots(self):
        return np.tile(self.Q.as_quat(), (2, 1))

    @property
    def is_pole(self):
        m = np.zeros(self.n, bool)
        m[self.n - self.n_pole:] = True
        return m

    def window_args(self, old):
        """(start_ns, dt_ns, t_next_win_beg_ns): every event old (the next window begins after them) or every event new"""
        return synth.T0_NS, DT_NS, T_EVENT_NS + (1 if old else 0)


def probe_table(Wp, Hp, Q, seed, z1=False):
    assert Wp % 4 == 0 and Hp % 4 == 0
    rng = np.random.default_rng(seed)
    sx, sy = Wp // 4, Hp // 4
    gy, gx = np.mgrid[0:sy, 0:sx]
    gx, gy = gx.ravel(), gy.ravel()
    border = (gx == 0) | (gx == sx - 1) | (gy == 0) | (gy == sy - 1)
    ok = np.ones(sx * sy, bool)
    axis = Q.apply([0.0, 0.0, 1.0])
    if z1:   # the whole slot (every target it can hold) within 75 degrees of the optical axis
        for ox in (0.0, 4.0):
            for oy in (0.0, 4.0):
                ok &= _ray(4.0 * gx + ox, 4.0 * gy + oy, Wp, Hp) @ axis > np.cos(np.deg2rad(75.0))
    poles = np.array([[0.0, 1.0, 0.0], [0.0, -1.0, 0.0]])
    if z1:
        poles = poles[poles @ axis > np.cos(np.deg2rad(75.0))]
    b_slots = np.flatnonzero(border & ok)
    i_slots = np.flatnonzero(~border & ok)
    # one event per sensor pixel; fewer where the 75-degree cone of a z = 1 table holds fewer slots than the sensor has pixels
    n_ev = min(N_PROBES, len(b_slots) + len(i_slots) + len(poles))
    n_ev -= n_ev % BATCH == 1          # no trailing one-event batch
    n = n_ev - len(poles)
    nb = min(n // 4, len(b_slots), n)
    nb = max(nb, n - len(i_slots))
    slots = np.concatenate([rng.choice(b_slots, nb, replace=False), rng.choice(i_slots, n - nb, replace=False)])
    slots = slots[rng.permutation(n)]
    cx, cy = gx[slots], gy[slots]
    ox = np.where(cx == sx - 1, rng.integers(0, 4, n), rng.integers(0, 2, n))
    oy = np.where(cy == sy - 1, rng.integers(0, 4, n), rng.integers(0, 2, n))

    def fracs(m):
        f = rng.uniform(0.02, 0.98, m)
        special = rng.random(m) < 0.1
        return np.where(special, rng.choice([1e-6, 1.0 - 1e-6, 0.5], m), f)

    fx_, fy_ = fracs(n), fracs(n)
    scale = rng.uniform(0.5, 3.0, n_ev)
    Rq = Q.as_matrix()
    for _ in range(20):
        target = np.stack([4.0 * cx + ox + fx_, 4.0 * cy + oy + fy_], -1)
        rays = np.concatenate([_ray(target[:, 0], target[:, 1], Wp, Hp), poles])
        b = Q.inv().apply(rays)
        b = b / b[:, 2:3] if z1 else b * scale[:, None]
        if z1:
            assert np.all(b[:, 2] == 1.0)
        close = probe_reference(b, Rq, Wp, Hp, n_pole=len(poles), check=False).dist[:n] < MIN_DIST
        if not close.any():
            break
        fx_[close], fy_[close] = rng.uniform(0.02, 0.98, close.sum()), rng.uniform(0.02, 0.98, close.sum())   # redraw
    else:
        raise AssertionError("probes within %g of an integer pixel coordinate after 20 redraws" % MIN_DIST)
    target = np.concatenate([target, np.full((len(poles), 2), np.nan)])
    lut = np.tile([0.0, 0.0, 1.0], (N_PROBES, 1))
    lut[:n_ev] = b
    for a in (lut, target):
        a.setflags(write=False)
    return ProbeTable(Wp, Hp, Q, z1, lut, target, len(poles), n_ev)


@dataclasses.dataclass
class ProbeRef:
    xx: np.ndarray      # vote cell (int64)
    yy: np.ndarray
    dx: np.ndarray      # bilinear offsets (float64, rounded from longdouble)
    dy: np.ndarray
    kept: np.ndarray    # 1 <= xx < Wp-2 && 1 <= yy < Hp-2
    dist: np.ndarray    # distance of (px, py) to the nearest integer coordinate, min over the two axes
    plane: np.ndarray   # Hp x Wp float64: the four weights of every kept probe
    mask: np.ndarray    # Hp x Wp bool: the pixels of kept probes' cells


def probe_reference(b, R, Wp, Hp, n_pole=2, check=True):
    """The votes of the table `b` (as stored: fp64) under the rotation R (3 x 3), projected in np.longdouble."""
    b = np.asarray(b, np.float64).astype(LD)
    R = np.asarray(R, np.float64).reshape(3, 3).astype(LD)
    r = b @ R.T
    x, y, z = r[:, 0], r[:, 1], r[:, 2]
    pi = LD("3.14159265358979323846264338327950288")
    fx, fy = Wp / (2 * pi), Hp / pi     # (Wp / 360) * 180 / pi: be_args' double differs by 1 ulp at most, 1e-13 of a pixel
    phi = np.arctan2(x, z)
    th = np.arcsin(np.clip(y / np.sqrt(x * x + y * y + z * z), -1, 1))
    px, py = LD(Wp) / 2 + phi * fx, LD(Hp) / 2 + th * fy
    xx, yy = np.trunc(px).astype(np.int64), np.trunc(py).astype(np.int64)     # (int): towards zero
    dx, dy = (px - xx).astype(np.float64), (py - yy).astype(np.float64)
    kept = (1 <= xx) & (xx < Wp - 2) & (1 <= yy) & (yy < Hp - 2)
    dist = np.minimum(np.abs(px - np.rint(px)), np.abs(py - np.rint(py))).astype(np.float64)
    n = len(b)
    plane = np.zeros((Hp, Wp))
    mask = np.zeros((Hp, Wp), bool)
    k = np.flatnonzero(kept)
    if check:
        assert not kept[n - n_pole:].any(), "a pole probe is kept"     # (row 0 or Hp - 1 / Hp: dropped by the border rule)
        assert np.all(dist[:n - n_pole] >= MIN_DIST), "a probe lies within %g of an integer pixel coordinate" % MIN_DIST
        cells = set()
        for i in k:   # disjoint cells
            for c in ((yy[i], xx[i]), (yy[i], xx[i] + 1), (yy[i] + 1, xx[i]), (yy[i] + 1, xx[i] + 1)):
                assert c not in cells, "cells of kept probes overlap at %s" % (c,)
                cells.add(c)
    for ox, oy, wgt in ((0, 0, (1 - dx) * (1 - dy)), (1, 0, dx * (1 - dy)), (0, 1, (1 - dx) * dy), (1, 1, dx * dy)):
        plane[yy[k] + oy, xx[k] + ox] = wgt[k]
        mask[yy[k] + oy, xx[k] + ox] = True
    return ProbeRef(xx, yy, dx, dy, kept, dist, plane, mask)


@functools.lru_cache(maxsize=None)
def probe_case(Wp, Hp, name, z1):
    """The table of one GPU case (read-only) and its reference under Q's own matrix."""
    seed = 7000 + 10 * list(PROBE_ORIENTATIONS).index(name) + (5 if z1 else 0) + Wp
    tab = probe_table(Wp, Hp, PROBE_ORIENTATIONS[name], seed, z1)
    return tab, probe_reference(tab.bearings, tab.Q.as_matrix(), Wp, Hp, tab.n_pole)


def describe(tab, ref, R, i):
    """One probe, for a failure message."""
    return ("probe %d (sensor pixel %d, %d): bearing %r, R %r, target %r, expected cell (%d, %d) dx %.9g dy %.9g, %s" %
            (i, i % SENSOR, i // SENSOR, tab.lut[i].tolist(), np.asarray(R).reshape(-1).tolist(), tab.target[i].tolist(),
             ref.xx[i], ref.yy[i], ref.dx[i], ref.dy[i], "kept" if ref.kept[i] else "dropped"))


def compare_plane(tab, ref, R, plane, tol):
    """Largest |plane - expected| over the kept cells; raises with the probe next to the first wrong pixel if a pixel outside
    the kept cells holds anything, a value is not finite or a cell is further than tol from its four weights."""
    plane = np.asarray(plane)
    assert plane.shape == ref.plane.shape
    bad = ~np.isfinite(plane)
    bad |= ~ref.mask & (plane != 0)
    diff = np.abs(plane.astype(np.float64) - ref.plane)
    bad |= ref.mask & ~(diff <= tol)
    if bad.any():
        py, px = np.argwhere(bad)[0]
        i = int(np.argmin(np.maximum(np.abs(ref.xx - px), np.abs(ref.yy - py))))
        y0, x0 = max(py - 2, 0), max(px - 2, 0)
        raise AssertionError("%d wrong pixels; first at (x %d, y %d): found %r, expected %r; nearest %s; found around it:\n%r" %
                             (bad.sum(), px, py, float(plane[py, px]), float(ref.plane[py, px]), describe(tab, ref, R, i),
                              plane[y0:py + 3, x0:px + 3]))
    return float(diff[ref.mask].max())


# ---------------------------------------------------------------- (c) far windows
def rotated(w, Q):
    """The window with its whole trajectory turned by Q (left-multiplied knots); the events stay."""
    turn = lambda k: (Q * Rot.from_quat(k)).as_quat()
    return dataclasses.replace(w, knots_true=turn(w.knots_true), knots_init=turn(w.knots_init))


@functools.lru_cache(maxsize=None)
def base_window(which):
    if which == "linear":
        return synth.backend_window(12_000, 120, 90, 100., 100., 59.5, 44.5, 256, 128, 2, 5, 1, 0.2, seed=5)
    return synth.backend_window(12_000, 120, 90, 100., 100., 59.5, 44.5, 256, 128, 4, 10, 3, 0.35, seed=5)


FAR = {
    "yaw90": Rot.from_euler("y", 90, degrees=True),
    "yaw180": Rot.from_euler("y", 180, degrees=True),
    "yaw-135": Rot.from_euler("y", -135, degrees=True),
    "pitch30": Rot.from_euler("x", 30, degrees=True),
    "pitch60": Rot.from_euler("x", 60, degrees=True),
    "pitch80": Rot.from_euler("x", 80, degrees=True),
    "pitch-80": Rot.from_euler("x", -80, degrees=True),
    "pitch90": Rot.from_euler("x", 90, degrees=True),
    "yaw180pitch45": Rot.from_euler("yx", [180, 45], degrees=True),
}
CUBIC_FAR = ["yaw180", "pitch80", "pitch30"]
FAR_CASES = [("linear", n) for n in FAR] + [("cubic", n) for n in CUBIC_FAR]
GLOBAL_MAP_FAR = ["yaw180", "pitch80"]


@functools.lru_cache(maxsize=None)
def far_window(which, name):
    return rotated(base_window(which), FAR[name])


def far_points(w):
    """The two evaluation points of test_gpu_backend.py's rules: drot = 0 and normal(0, 0.01)."""
    return [np.zeros(w.P), np.random.default_rng(4).normal(0, 0.01, w.P)]


def world_rays(w, knots=None):
    """R(t_i) * bearing_i of every event (unit vectors), by synth's own spline evaluation: the oracle-side geometry."""
    knots = w.knots_init if knots is None else knots
    R = synth.spline_rotations(w.order, knots, w.start_ns, w.dt_ns, w.t_ns)
    b = w.lut[w.y.astype(np.int64) * w.W + w.x]
    r = R.apply(b)
    return r / np.linalg.norm(r, axis=1, keepdims=True)
