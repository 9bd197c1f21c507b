"""Test helper: the gradient GATHER of the adjoint mode on the host in fp64 (numpy and oracle.pyoracle only, no GPU).

The adjoint gradient has two halves.  The image pass leaves the plane Jt (tests/dense_image_ops.py pins it per pixel); the gather
reads Jt at every event's vote cell, multiplies the two directional differences (A_e, B_e) by the event's pixel Jacobian, sums per
batch, maps every batch through its 3 x 3N spline Jacobian onto the knot parameters and the finalize forms (2/N)(S1 - mu S2).  This
file restates the second half with Jt AS AN INPUT, so that a device gradient can be held against it parameter by parameter:

  per event  front end: fe_warp_math<true>'s expressions in the reference's operation order (numpy never contracts), dx, dy, r0, r1
             cast to fp32 as the kernel casts them -- the vote cell is the device's bit for bit;
             back end / whole trajectory: R b, the equirectangular projection and dpm_ddrot in fp64, batch poses and Jacobian blocks
             from pyoracle.spline_eval (the Basalt vectors pin it), the blocks rounded to fp32 where Trajectory::evaluate rounds them;
  sums       S1_k = sum_e J_e,k . (A_e, B_e) with bilinear_grad's two differences of Jt, S2_k the same over the separable plane
             c = (Gy^T 1)(Gx^T 1)^T (dense_image_ops._operators) where border_grad's condition holds, everything in fp64;
             gradient = (2/N)(S1 - mu S2), mu the fp64 mean of dense_image_ops.blurred(A, sigma); MEAN_SQUARE has no mu term and
             GRADIENT_MAGNITUDE none either (the Sobel Jt of a constant is zero);
  M_k        the sum over the events of the magnitudes of the terms added into parameter k, with the same 2/N in front;
  bound_k    8 max(e32_k, 2^-24 M_k): e32_k is the distance of the SAME sums with the per-event factors evaluated as the kernels
             evaluate them -- A, B in fp32, c from fp32 factors, the entries of be_project<2> in fp32 from the fp64 ray, products
             widened to fp64, fp64 sums -- from the fp64 result.  dense_image_ops.bound's construction, taken per parameter; nothing
             measured on a device enters it.

An EventList is plain arrays, so a test can damage it on purpose (move one event to the next batch, drop one, skip one border term,
shift one batch's columns by a knot: MUTATIONS) and ask whether the damage exceeds bound_k (tests/test_gather_ref_cpu.py)."""
import copy
import math
from dataclasses import dataclass, field

import numpy as np

import dense_image_ops as dio
from oracle import iwe_numpy as inp
from oracle import pyoracle as po

F32 = np.float32
EPS32 = 2.0 ** -24
FACTOR = 8.0
CELL_MARGIN = 1e-9  # px: back-end cases keep every panorama coordinate this far from an integer (a thousand times the few ulp of
                    # the device's polynomial atan2 / asin at these focal lengths), so host and device choose the same vote cell


@dataclass
class EventList:
    """The voting events of one evaluation, in the device's order (time order, sampled), and the batches they belong to.

    J64 / J32: the event's 2 x 3 pixel Jacobian (row 0 multiplies A, row 1 multiplies B) in fp64 / as the kernel forms it in fp32.
    batch: index into Jb / col0.  Jb[b]: 3 x C block matrix of batch b (fp32 values held in fp64), C = 3 * order; col0[b]: the
    parameter its first column adds into (negative: columns below the num_fixed line, dropped).  The front end is one batch with
    Jb = I and col0 = 0."""
    W: int
    H: int
    P: int
    xx: np.ndarray
    yy: np.ndarray
    dx: np.ndarray
    dy: np.ndarray
    J64: np.ndarray
    J32: np.ndarray
    batch: np.ndarray
    Jb: np.ndarray
    col0: np.ndarray
    skip_s2: np.ndarray = None          # (mutation) events whose border term is left out
    margin: float = math.inf            # least distance of a panorama coordinate from an integer, all sampled events
    src: np.ndarray = None              # index of every voting event in the caller's event arrays
    dx64: np.ndarray = None             # the offsets before the cast to fp32 (forward_plane(exact=True) only)
    dy64: np.ndarray = None
    info: dict = field(default_factory=dict)

    def __post_init__(self):
        if self.skip_s2 is None:
            self.skip_s2 = np.zeros(len(self.xx), bool)

    @property
    def n(self):
        return len(self.xx)

    def batches_on(self, k):
        """the batches with a column on parameter k"""
        C = self.Jb.shape[2]
        return [int(b) for b in np.nonzero((self.col0 <= k) & (k < self.col0 + C))[0]]


# ---------------------------------------------------------------------------------------------------------------- front end
def device_int(u):
    """(int)u as the kernels' conversion instruction gives it: truncation, saturated to the int32 range, NaN -> 0 -- decided
    before any integer cast on the host (a ray with rz near zero gives |u| beyond every integer type)"""
    u = np.asarray(u, np.float64)
    lo, hi = -2.0 ** 31, 2.0 ** 31 - 1
    safe = np.clip(np.where(np.isnan(u), 0.0, u), lo, hi)
    return np.trunc(safe).astype(np.int64)


def fe_events(p, omega, batch=None):
    """EventList of a synth.FrontendPacket at angular velocity omega (fe_warp_math<true>, cmx_warp.hpp, operation for operation)"""
    batch = p.batch if batch is None else batch
    x, y, t = np.asarray(p.x, np.int64), np.asarray(p.y, np.int64), np.asarray(p.t_ns, np.int64)
    n = len(x)
    lut = np.asarray(p.lut, np.float64).reshape(-1, 3)
    wx, wy, wz = (float(v) for v in omega)
    nb = (n + batch - 1) // batch
    tref = inp._to_sec(p.t_ref_ns)
    dt_b = np.array([inp._to_sec(inp.batch_time_ns(t[b * batch], t[min((b + 1) * batch, n) - 1])) - tref for b in range(nb)])
    dt = dt_b[np.arange(n) // batch]
    b = lut[y * p.W + x]
    px, py, pz = b[:, 0], b[:, 1], b[:, 2]
    drx, dry, drz = wx * dt, wy * dt, wz * dt
    rx = px + (dry * pz - drz * py)
    ry = py + (drz * px - drx * pz)
    rz = pz + (drx * py - dry * px)
    with np.errstate(all="ignore"):  # (rz == 0, overflow past fp32 of an event that does not vote: the kernels' values as well)
        iz = 1.0 / rz
        cxn, cyn = rx * iz, ry * iz
        u = p.fx * cxn + p.cx
        v = p.fy * cyn + p.cy
        xx, yy = device_int(u), device_int(v)
        ok = (1 <= xx) & (xx < p.W - 2) & (1 <= yy) & (yy < p.H - 2)
        dx, dy = (u - xx).astype(F32), (v - yy).astype(F32)
        vx, vy, vz = (-dt) * px, (-dt) * py, (-dt) * pz
        a02, a12 = -cxn * iz, -cyn * iz
        r0 = np.stack([p.fx * (a02 * (-vy)), p.fx * (iz * (-vz) + a02 * vx), p.fx * (iz * vy)], axis=1).astype(F32)
        r1 = np.stack([p.fy * (iz * vz + a12 * (-vy)), p.fy * (a12 * vx), p.fy * (iz * (-vx))], axis=1).astype(F32)
    J = np.stack([r0, r1], axis=1)[ok]  # (n, 2, 3) fp32: the kernel holds r0, r1 in fp32 and widens the products
    return EventList(p.W, p.H, 3, xx[ok], yy[ok], dx[ok], dy[ok], J.astype(np.float64), J, np.zeros(int(ok.sum()), np.int64),
                     np.eye(3)[None], np.zeros(1, np.int64), src=np.nonzero(ok)[0], dx64=(u - xx)[ok], dy64=(v - yy)[ok],
                     info={"n_events": n, "batch": batch})


# ------------------------------------------------------------------------------------------------- back end, whole trajectory
def _dpm_ddrot64(x, y, z, fx, fy):
    """equirectangular_camera.h:33-44 times -[rb]x, all in fp64: (n, 2, 3)"""
    rho = np.sqrt(x * x + y * y + z * z)
    ydr, xdz = y / rho, x / z
    tmp1 = fx / ((1 + xdz * xdz) * z)
    tmp2 = -fy / np.sqrt(1 - ydr * ydr)
    tmp3 = ydr / (rho * rho)
    d00, d02 = tmp1, -tmp1 * xdz
    d10, d11, d12 = tmp2 * tmp3 * x, tmp2 * (tmp3 * y - 1 / rho), tmp2 * tmp3 * z
    return np.stack([np.stack([d02 * y, d00 * z + d02 * (-x), d00 * (-y)], axis=1),
                     np.stack([d11 * (-z) + d12 * y, d10 * z + d12 * (-x), d10 * (-y) + d11 * x], axis=1)], axis=1)


def _dpm_ddrot32(x, y, z, fx, fy):
    """be_project<2> (cmx_warp.hpp): the same entries in fp32 from the fp64 ray, operation for operation; the kernel's hardware
    reciprocals and reciprocal square root (1 ulp) stand here as correctly rounded fp32 divisions"""
    one = F32(1)
    rho = np.sqrt(x * x + y * y + z * z)
    xf, yf, zf, rhof = x.astype(F32), y.astype(F32), z.astype(F32), rho.astype(F32)
    fxf, fyf = F32(fx), F32(fy)
    inv_rho, inv_z = one / rhof, one / zf
    ydr, xdz = yf * inv_rho, xf * inv_z
    tmp1 = fxf * inv_z * (one / (one + xdz * xdz))
    tmp2 = -fyf * (one / np.sqrt(one - ydr * ydr))
    tmp3 = ydr * inv_rho * inv_rho
    d00, d02 = tmp1, -tmp1 * xdz
    d10, d11, d12 = tmp2 * tmp3 * xf, tmp2 * (tmp3 * yf - inv_rho), tmp2 * tmp3 * zf
    m = np.stack([np.stack([d02 * yf, d00 * zf + d02 * (-xf), d00 * (-yf)], axis=1),
                  np.stack([d11 * (-zf) + d12 * yf, d10 * zf + d12 * (-xf), d10 * (-yf) + d11 * xf], axis=1)], axis=1)
    assert m.dtype == F32
    return m


def be_events(x, y, t_ns, lut, W, Wp, Hp, order, knots, start_ns, dt_ns, num_fixed, batch, rate):
    """EventList of a back-end evaluation along `knots` (the control poses the evaluation uses: increments already applied).  The
    batch cursor, the shared batch time and the sampling stride are event_pano_warper.cpp's (oracle/iwe_numpy.backend_iwe)."""
    x, y, t = np.asarray(x, np.int64), np.asarray(y, np.int64), np.asarray(t_ns, np.int64)
    n = len(x)
    lut = np.asarray(lut, np.float64).reshape(-1, 3)
    K = len(knots)
    fx, fy = (Wp / 360.0) * 180.0 / math.pi, (Hp / 180.0) * 180.0 / math.pi
    cxp, cyp = Wp / 2.0, Hp / 2.0
    C = 3 * order
    cols, Jbs, col0, tb_list, segs = [], [], [], [], []
    margin = math.inf
    b0 = 0
    while b0 < n - 1:  # a trailing batch of ONE event is never warped
        b1 = b0 + batch if n - b0 > batch else n
        tb = inp.batch_time_ns(t[b0], t[b1 - 1])
        _, R, Jk, idx = po.spline_eval(order, knots, start_ns, dt_ns, tb, jac=True)
        sel = np.arange(b0, b1, rate)
        bv = lut[y[sel] * W + x[sel]]
        ray = (R[None, :, 0] * bv[:, 0:1] + R[None, :, 1] * bv[:, 1:2]) + R[None, :, 2] * bv[:, 2:3]
        rx, ry, rz = ray[:, 0], ray[:, 1], ray[:, 2]
        pxm = cxp + np.arctan2(rx, rz) * fx
        pym = cyp + np.arcsin(ry / np.sqrt(rx * rx + ry * ry + rz * rz)) * fy
        margin = min(margin, float(np.abs(pxm - np.rint(pxm)).min()), float(np.abs(pym - np.rint(pym)).min()))
        xx, yy = np.trunc(pxm).astype(np.int64), np.trunc(pym).astype(np.int64)
        ok = (1 <= xx) & (xx < Wp - 2) & (1 <= yy) & (yy < Hp - 2)
        bi = len(Jbs)
        cols.append((xx[ok], yy[ok], (pxm - xx).astype(F32)[ok], (pym - yy).astype(F32)[ok],
                     _dpm_ddrot64(rx[ok], ry[ok], rz[ok], fx, fy), _dpm_ddrot32(rx[ok], ry[ok], rz[ok], fx, fy),
                     np.full(int(ok.sum()), bi, np.int64), sel[ok], (pxm - xx)[ok], (pym - yy)[ok]))
        Jbs.append(np.concatenate([Jk[k].astype(F32) for k in range(order)], axis=1).astype(np.float64))  # 3 x 3N, fp32 values
        col0.append(3 * (idx - num_fixed))
        tb_list.append(tb)
        segs.append(idx)
        b0 += batch
    if not cols:
        z = np.zeros(0, np.int64)
        return EventList(Wp, Hp, 3 * (K - num_fixed), z, z, np.zeros(0, F32), np.zeros(0, F32), np.zeros((0, 2, 3)),
                         np.zeros((0, 2, 3), F32), z, np.zeros((0, 3, C)), z, src=z)
    cat = [np.concatenate([c[i] for c in cols]) for i in range(10)]
    return EventList(Wp, Hp, 3 * (K - num_fixed), cat[0], cat[1], cat[2], cat[3], cat[4], cat[5], cat[6], np.array(Jbs),
                     np.array(col0, np.int64), margin=margin, src=cat[7], dx64=cat[8], dy64=cat[9],
                     info={"batch_t": np.array(tb_list, np.int64), "segment": np.array(segs, np.int64), "n_events": n, "batch": batch,
                           "rate": rate, "order": order, "num_fixed": num_fixed})


def forward_plane(ev, exact=False):
    """The raw image of an EventList by voting on the host: fp32 weights from the fp32 offsets added in fp32, event by event (what
    a device plane is up to the order of its atomics), or -- exact -- fp64 weights from the fp64 offsets added in fp64 (the
    all-fp64 oracle's image)."""
    if exact:
        img = np.zeros((ev.H, ev.W))
        dx, dy = ev.dx64, ev.dy64
        w = np.stack([(1 - dx) * (1 - dy), dx * (1 - dy), (1 - dx) * dy, dx * dy], axis=1)
    else:
        img = np.zeros((ev.H, ev.W), F32)
        w = inp._weights(ev.dx, ev.dy)
    n = ev.n
    iy, ix = np.empty(4 * n, np.int64), np.empty(4 * n, np.int64)
    iy[0::4], iy[1::4], iy[2::4], iy[3::4] = ev.yy, ev.yy, ev.yy + 1, ev.yy + 1
    ix[0::4], ix[1::4], ix[2::4], ix[3::4] = ev.xx, ev.xx + 1, ev.xx, ev.xx + 1
    np.add.at(img, (iy, ix), w.reshape(-1))
    return img


# ------------------------------------------------------------------------------------------------------------------ the sums
def _differences(P00, P01, P10, P11, dx, dy, dtype):
    """bilinear_grad / border_grad: A = (1 - dy)(p01 - p00) + dy (p11 - p10), B = (1 - dx)(p10 - p00) + dx (p11 - p01)"""
    one = dtype(1)
    dx, dy = dx.astype(dtype), dy.astype(dtype)
    return (one - dy) * (P01 - P00) + dy * (P11 - P10), (one - dx) * (P10 - P00) + dx * (P11 - P01)


def gt1(H, W, sigma):
    """(Gy^T 1, Gx^T 1) in fp64 from dense_image_ops' operators"""
    if dio.radius(sigma) == 0:
        return np.ones(H), np.ones(W)
    o = dio._operators(H, W, sigma, np.float64)
    return (dio._dot(dio._T(o["Gy"]), np.ones((H, 1)))[:, 0], dio._dot(dio._T(o["Gx"]), np.ones((W, 1)))[:, 0])


def _scatter(ev, per_event):
    """per-event 3-vectors -> per-parameter sums: per batch, through the batch's block matrix, onto the parameters >= 0"""
    nb, _, C = ev.Jb.shape
    V = np.zeros((nb, 3))
    np.add.at(V, ev.batch, per_event)
    cols = np.einsum("bi,bic->bc", V, ev.Jb)
    k = ev.col0[:, None] + np.arange(C)[None, :]
    keep = (k >= 0) & (k < ev.P)
    out = np.zeros(ev.P)
    np.add.at(out, k[keep], cols[keep])
    return out


def _magnitudes(ev, per_event_abs):
    nb, _, C = ev.Jb.shape
    V = np.zeros((nb, 3))
    np.add.at(V, ev.batch, per_event_abs)
    cols = np.einsum("bi,bic->bc", V, np.abs(ev.Jb))
    k = ev.col0[:, None] + np.arange(C)[None, :]
    keep = (k >= 0) & (k < ev.P)
    out = np.zeros(ev.P)
    np.add.at(out, k[keep], cols[keep])
    return out


def _sums(ev, Jt, cy, cx, r, fp32):
    """(S1, S2, M1, M2) per parameter; fp32: the per-event factors as the kernels form them, products and sums in fp64 all the same"""
    dtype = F32 if fp32 else np.float64
    H, W = ev.H, ev.W
    xx, yy = ev.xx, ev.yy
    Jt = np.asarray(Jt, F32).astype(dtype)
    A, B = _differences(Jt[yy, xx], Jt[yy, xx + 1], Jt[yy + 1, xx], Jt[yy + 1, xx + 1], ev.dx, ev.dy, dtype)
    J = (ev.J32 if fp32 else ev.J64).astype(np.float64)
    A, B = A.astype(np.float64), B.astype(np.float64)
    S1 = _scatter(ev, A[:, None] * J[:, 0, :] + B[:, None] * J[:, 1, :])
    M1 = _magnitudes(ev, np.abs(A[:, None] * J[:, 0, :]) + np.abs(B[:, None] * J[:, 1, :]))
    edge = ((xx <= r) | (xx + 1 >= W - 1 - r) | (yy <= r) | (yy + 1 >= H - 1 - r)) & ~ev.skip_s2
    cxd, cyd = (cx.astype(F32), cy.astype(F32)) if fp32 else (cx, cy)  # (the device holds the factors in fp32: gt1_factors)
    ex, ey = xx[edge], yy[edge]
    Ac, Bc = _differences(cxd[ex] * cyd[ey], cxd[ex + 1] * cyd[ey], cxd[ex] * cyd[ey + 1], cxd[ex + 1] * cyd[ey + 1],
                          ev.dx[edge], ev.dy[edge], dtype)
    Ac, Bc = Ac.astype(np.float64), Bc.astype(np.float64)
    per = np.zeros((ev.n, 3))
    per[edge] = Ac[:, None] * J[edge, 0, :] + Bc[:, None] * J[edge, 1, :]
    mag = np.zeros((ev.n, 3))
    mag[edge] = np.abs(Ac[:, None] * J[edge, 0, :]) + np.abs(Bc[:, None] * J[edge, 1, :])
    return S1, _scatter(ev, per), M1, _magnitudes(ev, mag), int(edge.sum())


@dataclass
class GatherRef:
    g: np.ndarray       # (2/N)(S1 - mu S2), fp64
    bound: np.ndarray   # 8 max(e32, 2^-24 M) per parameter
    e32: np.ndarray     # |the fp32 restatement - g| per parameter
    M: np.ndarray       # sum of the magnitudes of the terms per parameter (with the 2/N)
    mu: float
    n_edge: int         # events whose border term is taken
    S1: np.ndarray
    S2: np.ndarray


def gather(ev, Jt, A, sigma, measure):
    """The reference gradient of an EventList over the plane Jt (fp32, as the device returned it), A the forward plane."""
    H, W = ev.H, ev.W
    Jt = np.asarray(Jt, F32)
    assert Jt.shape == (H, W), (Jt.shape, H, W)
    r = dio.radius(sigma)
    cy, cx = gt1(H, W, sigma)
    mu = float(dio.blurred(A, sigma).mean()) if measure == po.VARIANCE else 0.0
    scale = 2.0 / (W * H)
    S1, S2, M1, M2, n_edge = _sums(ev, Jt, cy, cx, r, False)
    T1, T2, _, _, _ = _sums(ev, Jt, cy, cx, r, True)
    g = scale * (S1 - mu * S2)
    e32 = np.abs(scale * (T1 - mu * T2) - g)
    M = scale * (M1 + abs(mu) * M2)
    return GatherRef(g, FACTOR * np.maximum(e32, EPS32 * M), e32, M, mu, n_edge, S1, S2)


def gather_value(ev, Jt, mu, sigma, measure):
    """only (2/N)(S1 - mu S2) of an EventList in fp64 (for a mutated list; mu is the unmutated reference's)"""
    cy, cx = gt1(ev.H, ev.W, sigma)
    S1, S2, _, _, _ = _sums(ev, np.asarray(Jt, F32), cy, cx, dio.radius(sigma), False)
    return 2.0 / (ev.W * ev.H) * (S1 - (mu if measure == po.VARIANCE else 0.0) * S2)


# --------------------------------------------------------------------------------------------------------------- comparison
def worst(dev, ref):
    """(parameter, device error over bound) of the worst parameter; a parameter with bound 0 must match exactly"""
    err = np.abs(np.asarray(dev, np.float64) - ref.g)
    ratio = np.where(ref.bound > 0, err / np.where(ref.bound > 0, ref.bound, 1.0), np.where(err > 0, np.inf, 0.0))
    k = int(np.argmax(ratio))
    return k, float(ratio[k])


def describe(ev, ref, dev, k, first_param=0):
    """names parameter k: the knot and component, the batches that reach it, both values"""
    nf = ev.info.get("num_fixed", 0)
    on = ev.batches_on(k)
    counts = np.bincount(ev.batch, minlength=len(ev.col0))
    where = ("parameter %d" % (k + first_param) if "order" not in ev.info else
             "parameter %d = knot %d component %d" % (k + first_param, nf + k // 3, k % 3))
    return ("%s; batches on it %s (voting events %s); device %.12g, reference %.12g, |difference| %.3e, bound %.3e, e32 %.3e, M %.3e"
            % (where, on[:8] + (["..."] if len(on) > 8 else []), [int(counts[b]) for b in on[:8]], dev[k], ref.g[k],
               abs(dev[k] - ref.g[k]), ref.bound[k], ref.e32[k], ref.M[k]))


# ---------------------------------------------------------------------------------------------------------------- mutations
def _copy(ev):
    out = copy.copy(ev)
    out.skip_s2 = ev.skip_s2.copy()
    return out


def weight(ev, Jt):
    """per event: the magnitude of what it adds to its batch's V (to choose an event whose loss is not accidentally nothing)"""
    Jt = np.asarray(Jt, np.float64)
    A, B = _differences(Jt[ev.yy, ev.xx], Jt[ev.yy, ev.xx + 1], Jt[ev.yy + 1, ev.xx], Jt[ev.yy + 1, ev.xx + 1], ev.dx, ev.dy,
                        np.float64)
    return np.abs(A[:, None] * ev.J64[:, 0, :] + B[:, None] * ev.J64[:, 1, :]).sum(axis=1)


def border_weight(ev, sigma):
    """per event: the magnitude of its border term (zero away from the band)"""
    cy, cx = gt1(ev.H, ev.W, sigma)
    xx, yy = ev.xx, ev.yy
    Ac, Bc = _differences(cx[xx] * cy[yy], cx[xx + 1] * cy[yy], cx[xx] * cy[yy + 1], cx[xx + 1] * cy[yy + 1], ev.dx, ev.dy, np.float64)
    return np.abs(Ac[:, None] * ev.J64[:, 0, :] + Bc[:, None] * ev.J64[:, 1, :]).sum(axis=1)


def mutate_next_batch(ev, e):
    """event e filed under the batch after its own (its geometry stays: what a segmented reduction does with a wrong run end)"""
    out = _copy(ev)
    out.batch = ev.batch.copy()
    assert ev.batch[e] + 1 < len(ev.col0), "the event sits in the last batch"
    out.batch[e] += 1
    return out


def mutate_drop(ev, e):
    out = _copy(ev)
    keep = np.ones(ev.n, bool)
    keep[e] = False
    for name in ("xx", "yy", "dx", "dy", "J64", "J32", "batch", "skip_s2", "src", "dx64", "dy64"):
        setattr(out, name, getattr(ev, name)[keep])
    return out


def mutate_skip_s2(ev, e):
    out = _copy(ev)
    out.skip_s2[e] = True
    return out


def mutate_shift_columns(ev, b):
    """batch b's columns land one knot further on"""
    out = _copy(ev)
    out.col0 = ev.col0.copy()
    out.col0[b] += 3
    return out


def corner_events(ev, r):
    """the events in the four r x r corners, where xx <= r (or its far-side form) AND yy <= r (or its far-side form)"""
    nx = (ev.xx <= r) | (ev.xx + 1 >= ev.W - 1 - r)
    ny = (ev.yy <= r) | (ev.yy + 1 >= ev.H - 1 - r)
    return np.nonzero(nx & ny)[0]
