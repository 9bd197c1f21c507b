#!/usr/bin/env python3
"""Timing of the time surfaces of a reconstruction (cmx_backend_recon_surface_*) -> profiles/recon_surface_timing.txt.

tools/time_recon_voxel.py's workload -- 20M events over 20 s from the event store (with polarity), 1280x720 sensor, 4096x2048
panorama, linear spline with 401 knots, batch 100 -- host clock around the synchronous calls, medians of --reps after --warmup, all
in ONE run:
    surface_add_from into 1000 by-polarity surfaces of 20 ms at 240x180 and at 640x480;
    view_add_from into frames of the same ranges, and voxel_add_from into signed 5-bin grids of the same ranges, both cut into the
    same sets over the same events;
    recon_add_from over the same events (the count panorama), for the ratios;
    decay_device and get_device of one surface and of a whole set, and the host forms of one surface;
    the route the calls replace: warp_from into host arrays (fp64 coordinates + flags, all events) plus a numpy maximum.at scatter of
    the events' timestamps into the surfaces, timed ONCE on the first --scatter-events events and SCALED to 20M, not measured there.
A surface set holds at most 2^28 cells and a voxel set at most 4096 planes and 2^28 cells, so the 1000 ranges are voted as several
sets -- the largest cut both kinds admit -- each over the events of its time range (cut at batch multiples); the row says how many.
Needs a GPU."""
import argparse
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402

import time_recon as tr  # noqa: E402  (the stream of the large configuration)
import time_recon_views as tv  # noqa: E402  (median_ms)

MAX_CELLS, MAX_PLANES, MAX_SURFACES = 1 << 28, 4096, 4096


def host_scatter(px, py, flags, t, pol, pano, views, Wv, Hv):
    """undo the equirectangular projection of the exported coordinates, re-project into each view, keep the latest timestamp"""
    from scipy.spatial.transform import Rotation as Rot
    Wp, Hp = pano
    cells = np.full((len(views), 2, Hv * Wv), -2 ** 63, np.int64)
    m = flags == 3
    phi, theta = (px[m] - Wp / 2.0) / (Wp / (2 * np.pi)), (py[m] - Hp / 2.0) / (Hp / np.pi)
    ray = np.stack([np.sin(phi) * np.cos(theta), np.sin(theta), np.cos(phi) * np.cos(theta)], axis=1)
    tm, ch = t[m], np.where(pol[m] != 0, 0, 1)
    for k, g in enumerate(views):
        s = (tm >= g.t_lo_ns) & (tm < g.t_hi_ns)
        if not s.any():
            continue
        c = ray[s] @ Rot.from_quat(np.array(g.quat_xyzw)).as_matrix()  # R^T ray, row by row
        with np.errstate(divide="ignore", invalid="ignore"):
            u, w = g.fx * (c[:, 0] / c[:, 2]) + g.cx, g.fy * (c[:, 1] / c[:, 2]) + g.cy
            ok = (c[:, 2] > 0) & (u >= 1) & (u < Wv - 2) & (w >= 1) & (w < Hv - 2)
        cx, cy = (u[ok] + 0.5).astype(np.int64), (w[ok] + 0.5).astype(np.int64)
        np.maximum.at(cells[k], (ch[s][ok], cy * Wv + cx), tm[s][ok])
    return cells


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--events", type=int, default=20_000_000)
    ap.add_argument("--seconds", type=float, default=20.0)
    ap.add_argument("--sensor", type=int, nargs=2, default=(1280, 720))
    ap.add_argument("--pano", type=int, nargs=2, default=(4096, 2048))
    ap.add_argument("--batch", type=int, default=100)
    ap.add_argument("--surface-ms", type=float, default=20.0)
    ap.add_argument("--bins", type=int, default=5)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--scatter-events", type=int, default=1_000_000)
    ap.add_argument("--commit", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "recon_surface_timing.txt"))
    a = ap.parse_args()
    from cmax_slam_amd import _lib, evaluator, trajectory
    L = _lib.lib()
    assert L.cmx_device_count() > 0, "no GPU visible: this tool measures on the device only"
    commit = a.commit
    if not commit:
        try:
            commit = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], stderr=subprocess.DEVNULL).decode().strip()
        except Exception:
            commit = "unknown"
    x, y, t, knots, start_ns, dt_ns, lut = tr.make_inputs(a)
    n = len(x)
    pol = np.random.default_rng(12).integers(0, 2, n).astype(np.uint8)
    W, H = a.sensor
    Wp, Hp = a.pano
    f = 0.9 * W  # (time_recon.make_inputs' focal length)
    store = evaluator.EventStore(W, H, n)
    store.push(x, y, t, polarity=pol)
    be = evaluator.BackendEvaluator(W, H, lut, Wp, Hp)
    be.reconstruct_begin(2, knots, start_ns, dt_ns, a.batch, 1)
    period = int(round(a.surface_ms * 1e6))
    B = a.bins

    def views_of(Wv, Hv):
        return trajectory.frame_views(2, knots, start_ns, dt_ns, period, (f * Wv / W, f * Hv / H, 0.5 * (Wv - 1), 0.5 * (Hv - 1)))

    def per_set(Wv, Hv):  # the largest cut a by-polarity surface set AND a voxel set of B bins admit
        return max(1, min(MAX_CELLS // (Wv * Hv * 2), MAX_SURFACES, MAX_CELLS // (Wv * Hv * B), MAX_PLANES // B))

    rows = []

    def measure(Wv, Hv):
        views = views_of(Wv, Hv)
        per = per_set(Wv, Hv)
        parts = [views[i:i + per] for i in range(0, len(views), per)]
        ms = {"surface": [0.0, 0.0], "view": [0.0, 0.0], "voxel": [0.0, 0.0]}
        votes = {"surface": 0, "view": 0, "voxel": 0}
        for part in parts:
            i0 = int(np.searchsorted(t, min(g.t_lo_ns for g in part)) // a.batch * a.batch)
            i1 = int(min(n, -(-int(np.searchsorted(t, max(g.t_hi_ns for g in part))) // a.batch) * a.batch))
            cnt = np.zeros(len(part), np.int64)  # (the counters alone: nothing else crosses the bus)
            kinds = (("surface", lambda: be.reconstruct_surface_begin(part, Wv, Hv, by_polarity=True), be.reconstruct_surface_add_from,
                      be.reconstruct_surface_reset, L.cmx_backend_recon_surface_get, be.reconstruct_surface_end),
                     ("view", lambda: be.reconstruct_view_begin(part, Wv, Hv), be.reconstruct_view_add_from,
                      be.reconstruct_view_reset, L.cmx_backend_recon_view_get, be.reconstruct_view_end),
                     ("voxel", lambda: be.reconstruct_voxel_begin(part, Wv, Hv, B, signed=True), be.reconstruct_voxel_add_from,
                      be.reconstruct_voxel_reset, L.cmx_backend_recon_voxel_get, be.reconstruct_voxel_end))
            for kind, begin, add_from, reset, get, end in kinds:
                begin()
                med, lo = tv.median_ms(lambda: add_from(store, i0, i1 - i0), a.warmup, a.reps)
                ms[kind][0] += med
                ms[kind][1] += lo
                reset()
                add_from(store, i0, i1 - i0)
                be._ck(get(be._ctx, 0, len(part), None, cnt.ctypes.data_as(_lib.c_i64p)))
                votes[kind] += int(cnt.sum())
                end()
        rows.append((len(views), Wv, Hv, len(parts), ms, votes))

    add = tv.median_ms(lambda: be.reconstruct_add_from(store, 0, n), a.warmup, a.reps)
    measure(240, 180)
    measure(640, 480)
    add_after = tv.median_ms(lambda: be.reconstruct_add_from(store, 0, n), a.warmup, a.reps)

    # the surfaces' way out: one surface and a whole set, decayed and as they are, into device memory; one surface to the host
    import torch
    out_rows = []
    tau = float(period)
    for Wv, Hv in ((240, 180), (640, 480)):
        vs = views_of(Wv, Hv)[:per_set(Wv, Hv)]
        be.reconstruct_surface_begin(vs, Wv, Hv, by_polarity=True)
        be.reconstruct_surface_add_from(store, 0, n)
        k = len(vs) // 2
        one_f = torch.empty((1, 2, Hv, Wv), dtype=torch.float32, device="cuda")
        all_f = torch.empty((len(vs), 2, Hv, Wv), dtype=torch.float32, device="cuda")
        one_i = torch.empty((1, 2, Hv, Wv), dtype=torch.int64, device="cuda")
        all_i = torch.empty((len(vs), 2, Hv, Wv), dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        out_rows.append((Wv, Hv, len(vs),
                         tv.median_ms(lambda: be.reconstruct_surface_decay(tau, None, k, 1, out=one_f), a.warmup, a.reps),
                         tv.median_ms(lambda: be.reconstruct_surface_decay(tau, out=all_f), a.warmup, a.reps),
                         tv.median_ms(lambda: be.reconstruct_surface_get(k, 1, out=one_i), a.warmup, a.reps),
                         tv.median_ms(lambda: be.reconstruct_surface_get(out=all_i), a.warmup, a.reps),
                         tv.median_ms(lambda: be.reconstruct_surface_decay(tau, None, k, 1), a.warmup, a.reps),
                         tv.median_ms(lambda: be.reconstruct_surface_get(k, 1), a.warmup, a.reps)))
        del one_f, all_f, one_i, all_i
        be.reconstruct_surface_end()

    # the route the calls replace: export every event's coordinates to the host, undo the projection, re-project, scatter
    xy, fl = np.zeros((n, 2)), np.zeros(n, np.uint8)  # (touched: no first-touch page faults inside the timed call)

    def export():
        be._ck(L.cmx_backend_recon_warp_from(be._ctx, store._h, 0, n, _lib.WARP_F64, xy.ctypes.data, fl.ctypes.data))
    warp = tv.median_ms(export, a.warmup, max(3, a.reps // 3))
    ns = min(a.scatter_events, n)
    vs = [g for g in views_of(240, 180) if g.t_lo_ns <= t[ns - 1]]
    t0 = time.perf_counter()
    host_scatter(xy[:ns, 0], xy[:ns, 1], fl[:ns], t[:ns], pol[:ns], a.pano, vs, 240, 180)
    scatter_ms = 1e3 * (time.perf_counter() - t0)
    be.reconstruct_end()
    be.close()
    store.close()

    Ls = ["time surfaces of a reconstruction: cmx_backend_recon_surface_add_from / _surface_get* / _surface_decay*",
          "commit %s; %d events over %.0f s from the event store (with polarity), sensor %dx%d, panorama %dx%d, linear spline of %d "
          "knots, batch %d, default mode" % (commit, n, a.seconds, W, H, Wp, Hp, len(knots), a.batch),
          "host clock around synchronous calls, ms: median (min) of %d after %d warm-up calls, one run" % (a.reps, a.warmup), "",
          "recon_add_from over the %d events (the count panorama), before / after the rows below   %8.3f (%.3f) / %8.3f (%.3f)" %
          ((n,) + add + add_after), "",
          "by-polarity surfaces of %.0f ms against frames (view_add_from) and signed grids of %d bins (voxel_add_from) of the same ranges: "
          "same sets, same events, this run" % (a.surface_ms, B),
          "  ranges    size    sets   surface_add_from ms (min)   view_add_from ms (min)   voxel_add_from ms (min)   surface / view   / voxel   "
          "/ add_from   events voted: surfaces (views, grids)"]
    for nv, Wv, Hv, parts, ms, votes in rows:
        s, v, g = ms["surface"], ms["view"], ms["voxel"]
        Ls.append("  %5d  %4dx%-4d   %3d       %8.3f (%.3f)          %8.3f (%.3f)         %8.3f (%.3f)         %5.2fx        %5.2fx     %5.2fx     "
                  "%d (%d, %d)" % (nv, Wv, Hv, parts, s[0], s[1], v[0], v[1], g[0], g[1], s[0] / v[0], s[0] / g[0], s[0] / add[0],
                                   votes["surface"], votes["view"], votes["voxel"]))
    Ls += ["", "the surfaces' way out, tau = %.0f ms    surfaces in the set   decay_device, one   decay_device, the set   get_device, one   "
           "get_device, the set   decay -> host, one   get -> host, one" % a.surface_ms]
    for row in out_rows:
        Wv, Hv, nv = row[:3]
        Ls.append("  %4dx%-4d x 2 channels                     %5d        " % (Wv, Hv, nv) +
                  "   ".join("%8.3f (%.3f)" % r for r in row[3:]))
    Ls += ["", "the route these calls replace: per-event export to the host, re-projection and scatter there",
           "  warp_from, fp64 coordinates + flags of all %d events into host arrays                  %8.3f (%.3f)" % ((n,) + warp),
           "  numpy: undo the projection, re-project, maximum.at of the FIRST %d events into %d surfaces of 240x180 x 2, once   %8.1f   "
           "(SCALED, not measured: %.1f s per 20M at that rate)" % (ns, len(vs), scatter_ms, scatter_ms * 20e6 / ns * 1e-3)]
    text = "\n".join(Ls) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
