#!/usr/bin/env python3
"""Timing of the voxel grids of a reconstruction (cmx_backend_recon_voxel_*) -> profiles/recon_voxel_timing.txt.

tools/time_recon.py's large configuration -- 20M events over 20 s from the event store (with polarity), 1280x720 sensor,
4096x2048 panorama, linear spline with 401 knots, batch 100 -- host clock around the synchronous calls, medians of --reps after
--warmup, all in ONE run:
    voxel_add_from into 1000 signed grids of 20 ms x 5 bins at 240x180 and at 640x480;
    the baseline, view_add_from into 1000 frames of the same ranges, cut into the same sets over the same events;
    recon_add_from over the same events (the count panorama);
    voxel_get of one grid into a host array, and voxel_get_device of one grid and of a whole set into device memory;
    the route the calls replace: warp_from into host arrays (fp64 coordinates + flags, all events) plus a numpy scatter of the
    2 x 4 weighted votes per event into the grids, timed ONCE on the first --scatter-events events (it takes seconds at 20M).
A voxel set holds at most 4096 planes and 2^28 cells, so the 1000 grids are voted as several sets, each over the events of its
time range (cut at batch multiples); the row says how many.  Needs a GPU."""
import argparse
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402

import time_recon as tr  # noqa: E402  (the stream of the large configuration)
import time_recon_views as tv  # noqa: E402  (median_ms)

MAX_CELLS, MAX_PLANES = 1 << 28, 4096


def host_scatter(px, py, flags, t, pol, pano, grids, Wv, Hv, n_bins):
    """undo the equirectangular projection of the exported coordinates, re-project into each grid, scatter the 2 x 4 signed votes"""
    from scipy.spatial.transform import Rotation as Rot
    Wp, Hp = pano
    vol = np.zeros((len(grids), n_bins, Hv * Wv), np.float32)
    m = flags == 3
    phi, theta = (px[m] - Wp / 2.0) / (Wp / (2 * np.pi)), (py[m] - Hp / 2.0) / (Hp / np.pi)
    ray = np.stack([np.sin(phi) * np.cos(theta), np.sin(theta), np.cos(phi) * np.cos(theta)], axis=1)
    tm, sg = t[m], np.where(pol[m] != 0, np.float32(1), np.float32(-1))
    one = np.float32(1)
    for k, g in enumerate(grids):
        s = (tm >= g.t_lo_ns) & (tm < g.t_hi_ns)
        if not s.any():
            continue
        c = ray[s] @ Rot.from_quat(np.array(g.quat_xyzw)).as_matrix()  # R^T ray, row by row
        with np.errstate(divide="ignore", invalid="ignore"):
            u, w = g.fx * (c[:, 0] / c[:, 2]) + g.cx, g.fy * (c[:, 1] / c[:, 2]) + g.cy
            ok = (c[:, 2] > 0) & (u >= 1) & (u < Wv - 2) & (w >= 1) & (w < Hv - 2)
        u, w = u[ok], w[ok]
        xx, yy = u.astype(np.int64), w.astype(np.int64)
        dx, dy = (u - xx).astype(np.float32), (w - yy).astype(np.float32)
        tau = (tm[s][ok] - g.t_lo_ns).astype(np.float64) * ((n_bins - 1) / float(g.t_hi_ns - g.t_lo_ns))
        b0 = np.minimum(tau.astype(np.int64), n_bins - 2)
        f = (tau - b0).astype(np.float32)
        sgn = sg[s][ok]
        for b, wt in ((b0, one - f), (b0 + 1, f)):
            for wb, oy, ox in (((one - dx) * (one - dy), 0, 0), (dx * (one - dy), 0, 1), ((one - dx) * dy, 1, 0), (dx * dy, 1, 1)):
                np.add.at(vol[k], (b, (yy + oy) * Wv + (xx + ox)), sgn * (wt * wb))
    return vol


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--events", type=int, default=20_000_000)
    ap.add_argument("--seconds", type=float, default=20.0)
    ap.add_argument("--sensor", type=int, nargs=2, default=(1280, 720))
    ap.add_argument("--pano", type=int, nargs=2, default=(4096, 2048))
    ap.add_argument("--batch", type=int, default=100)
    ap.add_argument("--grid-ms", type=float, default=20.0)
    ap.add_argument("--bins", type=int, default=5)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--scatter-events", type=int, default=1_000_000)
    ap.add_argument("--commit", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "recon_voxel_timing.txt"))
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
    period = int(round(a.grid_ms * 1e6))
    B = a.bins

    def grids_of(Wv, Hv):
        return trajectory.voxel_grids(2, knots, start_ns, dt_ns, period, (f * Wv / W, f * Hv / H, 0.5 * (Wv - 1), 0.5 * (Hv - 1)))

    rows = []

    def measure(Wv, Hv):
        """voxel_add_from and view_add_from over all events, the 1000 grids cut into sets of at most 4096 planes and 2^28 cells"""
        grids = grids_of(Wv, Hv)
        per = max(1, min(MAX_CELLS // (Wv * Hv * B), MAX_PLANES // B))
        parts = [grids[i:i + per] for i in range(0, len(grids), per)]
        vox, view, votes, frame_votes = [0.0, 0.0], [0.0, 0.0], 0, 0
        for part in parts:
            i0 = int(np.searchsorted(t, min(g.t_lo_ns for g in part)) // a.batch * a.batch)
            i1 = int(min(n, -(-int(np.searchsorted(t, max(g.t_hi_ns for g in part))) // a.batch) * a.batch))
            be.reconstruct_voxel_begin(part, Wv, Hv, B, signed=True)
            med, lo = tv.median_ms(lambda: be.reconstruct_voxel_add_from(store, i0, i1 - i0), a.warmup, a.reps)
            vox[0] += med
            vox[1] += lo
            be.reconstruct_voxel_reset()
            be.reconstruct_voxel_add_from(store, i0, i1 - i0)
            cnt = np.zeros(len(part), np.int64)  # (the counters alone: no plane crosses the bus)
            be._ck(L.cmx_backend_recon_voxel_get(be._ctx, 0, len(part), None, cnt.ctypes.data_as(_lib.c_i64p)))
            votes += int(cnt.sum())
            be.reconstruct_voxel_end()
            be.reconstruct_view_begin(part, Wv, Hv)
            med, lo = tv.median_ms(lambda: be.reconstruct_view_add_from(store, i0, i1 - i0), a.warmup, a.reps)
            view[0] += med
            view[1] += lo
            be.reconstruct_view_reset()
            be.reconstruct_view_add_from(store, i0, i1 - i0)
            be._ck(L.cmx_backend_recon_view_get(be._ctx, 0, len(part), None, cnt.ctypes.data_as(_lib.c_i64p)))
            frame_votes += int(cnt.sum())
            be.reconstruct_view_end()
        rows.append((len(grids), Wv, Hv, len(parts), vox, view, votes, frame_votes))

    add = tv.median_ms(lambda: be.reconstruct_add_from(store, 0, n), a.warmup, a.reps)
    measure(240, 180)
    measure(640, 480)
    add_after = tv.median_ms(lambda: be.reconstruct_add_from(store, 0, n), a.warmup, a.reps)

    # the volumes' way out: one grid to the host, one grid and a whole set into device memory
    import torch
    out_rows = []
    for Wv, Hv in ((240, 180), (640, 480)):
        gs = grids_of(Wv, Hv)[:max(1, min(MAX_CELLS // (Wv * Hv * B), MAX_PLANES // B))]
        be.reconstruct_voxel_begin(gs, Wv, Hv, B, signed=True)
        be.reconstruct_voxel_add_from(store, 0, n)
        k = len(gs) // 2
        one = torch.empty((1, B, Hv, Wv), dtype=torch.float32, device="cuda")
        every = torch.empty((len(gs), B, Hv, Wv), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        out_rows.append((Wv, Hv, len(gs), tv.median_ms(lambda: be.reconstruct_voxel_get(k, 1), a.warmup, a.reps),
                         tv.median_ms(lambda: be.reconstruct_voxel_get(k, 1, out=one), a.warmup, a.reps),
                         tv.median_ms(lambda: be.reconstruct_voxel_get(out=every), a.warmup, a.reps)))
        del one, every
        be.reconstruct_voxel_end()

    # the route the calls replace: export every event's coordinates to the host, undo the projection, re-project, scatter
    xy, fl = np.zeros((n, 2)), np.zeros(n, np.uint8)  # (touched: no first-touch page faults inside the timed call)

    def export():
        be._ck(L.cmx_backend_recon_warp_from(be._ctx, store._h, 0, n, _lib.WARP_F64, xy.ctypes.data, fl.ctypes.data))
    warp = tv.median_ms(export, a.warmup, max(3, a.reps // 3))
    ns = min(a.scatter_events, n)
    gs = [g for g in grids_of(240, 180) if g.t_lo_ns <= t[ns - 1]]
    t0 = time.perf_counter()
    host_scatter(xy[:ns, 0], xy[:ns, 1], fl[:ns], t[:ns], pol[:ns], a.pano, gs, 240, 180, B)
    scatter_ms = 1e3 * (time.perf_counter() - t0)
    be.reconstruct_end()
    be.close()
    store.close()

    Ls = ["voxel grids of a reconstruction: cmx_backend_recon_voxel_add_from / _voxel_get / _voxel_get_device",
          "commit %s; %d events over %.0f s from the event store (with polarity), sensor %dx%d, panorama %dx%d, linear spline of %d "
          "knots, batch %d, default mode" % (commit, n, a.seconds, W, H, Wp, Hp, len(knots), a.batch),
          "host clock around synchronous calls, ms: median (min) of %d after %d warm-up calls, one run" % (a.reps, a.warmup), "",
          "recon_add_from over the %d events (the count panorama), before / after the rows below   %8.3f (%.3f) / %8.3f (%.3f)" %
          ((n,) + add + add_after), "",
          "signed grids of %.0f ms x %d bins against frames of the same ranges (the baseline: view_add_from, same sets, same events, this run)"
          % (a.grid_ms, B),
          "  grids     size    sets   voxel_add_from ms (min)   view_add_from ms (min)   voxel / view   / add_from   events voted (views)"]
    for ng, Wv, Hv, parts, vox, view, votes, fv in rows:
        Ls.append("  %5d  %4dx%-4d   %3d      %8.3f (%.3f)        %8.3f (%.3f)         %5.2fx       %5.2fx     %d (%d)" %
                  (ng, Wv, Hv, parts, vox[0], vox[1], view[0], view[1], vox[0] / view[0], vox[0] / add[0], votes, fv))
    Ls += ["", "the volumes' way out               grids in the set   voxel_get, one grid -> host   get_device, one grid   get_device, the set"]
    for Wv, Hv, ng, g1, d1, dall in out_rows:
        Ls.append("  %4dx%-4d x %d bins                    %5d            %8.3f (%.3f)        %8.3f (%.3f)      %8.3f (%.3f)" %
                  ((Wv, Hv, B, ng) + g1 + d1 + dall))
    Ls += ["", "the route these calls replace: per-event export to the host, re-projection and scatter there",
           "  warp_from, fp64 coordinates + flags of all %d events into host arrays                  %8.3f (%.3f)" % ((n,) + warp),
           "  numpy: undo the projection, re-project, scatter the FIRST %d events into %d grids of 240x180 x %d, once   %8.1f   "
           "(%.1f s per 20M at that rate)" % (ns, len(gs), B, scatter_ms, scatter_ms * 20e6 / ns * 1e-3)]
    text = "\n".join(Ls) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
