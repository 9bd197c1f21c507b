#!/usr/bin/env python3
"""Timing of the pinhole views of a reconstruction (cmx_backend_recon_view_*) -> profiles/recon_views_timing.txt.

tools/time_recon.py's large configuration -- 20M events over 20 s from the event store, 1280x720 sensor, 4096x2048 panorama, linear
spline with 401 knots, batch 100 -- host clock around the synchronous calls, medians of --reps after --warmup, all in one run and
all beside recon_add_from over the same events:
    one all-time view of 640x480; 1000 disjoint frames of 20 ms at 240x180 -- alone, and in a table of 4096 views of which the
    other 3096 meet no event -- and at 640x480; the same frames exposed for twice their
    period (every event votes into two views); one crop of 1024x1024; view_get and view_render of one frame;
    the route the calls replace: warp_from into host arrays (fp64 coordinates + flags, all events) plus a numpy scatter of the
    bilinear votes into the frames, timed on the first --scatter-events events only (it takes seconds at 20M).
A view set holds at most 2^28 cells, so the 1000 frames of 640x480 are voted as two sets of 500, each over its half of the events.
Needs a GPU."""
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

MAX_CELLS = 1 << 28


def median_ms(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    v = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        v.append(1e3 * (time.perf_counter() - t0))
    return statistics.median(v), min(v)


def host_scatter(px, py, flags, t, pano, views, Wv, Hv):
    """undo the equirectangular projection of the exported coordinates, re-project into each frame, scatter the bilinear votes"""
    from scipy.spatial.transform import Rotation as Rot
    Wp, Hp = pano
    planes = np.zeros((len(views), Hv * Wv), np.float32)
    m = flags == 3
    phi, theta = (px[m] - Wp / 2.0) / (Wp / (2 * np.pi)), (py[m] - Hp / 2.0) / (Hp / np.pi)
    ray = np.stack([np.sin(phi) * np.cos(theta), np.sin(theta), np.cos(phi) * np.cos(theta)], axis=1)
    tm = t[m]
    one = np.float32(1)
    for k, v in enumerate(views):
        s = (tm >= v.t_lo_ns) & (tm < v.t_hi_ns)
        if not s.any():
            continue
        c = ray[s] @ Rot.from_quat(np.array(v.quat_xyzw)).as_matrix()  # R^T ray, row by row
        with np.errstate(divide="ignore", invalid="ignore"):
            u, w = v.fx * (c[:, 0] / c[:, 2]) + v.cx, v.fy * (c[:, 1] / c[:, 2]) + v.cy
            ok = (c[:, 2] > 0) & (u >= 1) & (u < Wv - 2) & (w >= 1) & (w < Hv - 2)
        u, w = u[ok], w[ok]
        xx, yy = u.astype(np.int64), w.astype(np.int64)
        dx, dy = (u - xx).astype(np.float32), (w - yy).astype(np.float32)
        for wt, oy, ox in (((one - dx) * (one - dy), 0, 0), (dx * (one - dy), 0, 1), ((one - dx) * dy, 1, 0), (dx * dy, 1, 1)):
            np.add.at(planes[k], (yy + oy) * Wv + (xx + ox), wt)
    return planes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--events", type=int, default=20_000_000)
    ap.add_argument("--seconds", type=float, default=20.0)
    ap.add_argument("--sensor", type=int, nargs=2, default=(1280, 720))
    ap.add_argument("--pano", type=int, nargs=2, default=(4096, 2048))
    ap.add_argument("--batch", type=int, default=100)
    ap.add_argument("--frame-ms", type=float, default=20.0)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--scatter-events", type=int, default=1_000_000)
    ap.add_argument("--commit", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "recon_views_timing.txt"))
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
    W, H = a.sensor
    Wp, Hp = a.pano
    f = 0.9 * W  # (time_recon.make_inputs' focal length)
    store = evaluator.EventStore(W, H, n)
    store.push(x, y, t)
    be = evaluator.BackendEvaluator(W, H, lut, Wp, Hp)
    be.reconstruct_begin(2, knots, start_ns, dt_ns, a.batch, 1)
    period = int(round(a.frame_ms * 1e6))

    def intr(Wv, Hv):
        return f * Wv / W, f * Hv / H, 0.5 * (Wv - 1), 0.5 * (Hv - 1)

    def frames(Wv, Hv, exposure=None):
        return trajectory.frame_views(2, knots, start_ns, dt_ns, period, intr(Wv, Hv), exposure_ns=exposure)

    rows = []

    def measure(label, views, Wv, Hv):
        """view_add_from over all events, the set split where it exceeds 2^28 cells (each part over the events of its time range)"""
        per = max(1, MAX_CELLS // (Wv * Hv))
        parts = [views[i:i + per] for i in range(0, len(views), per)]
        total, total_min, votes = 0.0, 0.0, 0
        for part in parts:
            if len(parts) == 1:
                i0, i1 = 0, n
            else:
                i0 = int(np.searchsorted(t, min(v.t_lo_ns for v in part)) // a.batch * a.batch)
                i1 = int(min(n, -(-int(np.searchsorted(t, max(v.t_hi_ns for v in part))) // a.batch) * a.batch))
            be.reconstruct_view_begin(part, Wv, Hv)
            med, lo = median_ms(lambda: be.reconstruct_view_add_from(store, i0, i1 - i0), a.warmup, a.reps)
            be.reconstruct_view_reset()
            be.reconstruct_view_add_from(store, i0, i1 - i0)
            cnt = np.zeros(len(part), np.int64)  # (the counters alone: no plane crosses the bus)
            be._ck(L.cmx_backend_recon_view_get(be._ctx, 0, len(part), None, cnt.ctypes.data_as(_lib.c_i64p)))
            votes += int(cnt.sum())
            total += med
            total_min += lo
        rows.append((label, len(views), Wv, Hv, len(parts), total, total_min, votes))
        return total

    add = median_ms(lambda: be.reconstruct_add_from(store, 0, n), a.warmup, a.reps)
    measure("one all-time view", [trajectory.crop_view(knots[len(knots) // 2], 58.0, 640, 480)], 640, 480)
    measure("disjoint frames", frames(240, 180), 240, 180)
    # the same frames in a table four times as long: 3096 more views whose ranges lie behind the recording and meet no run.  Were a
    # view looked at per event, this row would cost a multiple of the one above; it costs the longer scan per workgroup
    t_end = int(t[-1]) + 1
    dead = [_lib.recon_view(knots[0], *intr(240, 180), t_end + k * period, t_end + (k + 1) * period) for k in range(4096 - 1000)]
    measure("... among 4096 views (3096 never met)", frames(240, 180) + dead, 240, 180)
    measure("disjoint frames", frames(640, 480), 640, 480)
    measure("frames, exposure 2 x period", frames(240, 180, 2 * period), 240, 180)
    measure("frames, exposure 2 x period", frames(640, 480, 2 * period), 640, 480)
    measure("one crop", [trajectory.crop_view(knots[len(knots) // 2], 15.0, 1024, 1024)], 1024, 1024)
    add_after = median_ms(lambda: be.reconstruct_add_from(store, 0, n), a.warmup, a.reps)

    # view_get / view_render of one frame, out of a set that has been voted
    per_frame = {}
    for Wv, Hv in ((240, 180), (640, 480)):
        vs = frames(Wv, Hv)[:min(800, MAX_CELLS // (Wv * Hv))]
        be.reconstruct_view_begin(vs, Wv, Hv)
        be.reconstruct_view_add_from(store, 0, n)
        k = len(vs) // 2
        per_frame[(Wv, Hv)] = (median_ms(lambda: be.reconstruct_view_get(k, 1), a.warmup, a.reps),
                               median_ms(lambda: be.reconstruct_view_render(k, 0.75), a.warmup, a.reps))
    be.reconstruct_view_end()

    # the route the calls replace: export every event's coordinates to the host, undo the projection, re-project, scatter
    xy, fl = np.zeros((n, 2)), np.zeros(n, np.uint8)  # (touched: no first-touch page faults inside the timed call)

    def export():
        be._ck(L.cmx_backend_recon_warp_from(be._ctx, store._h, 0, n, _lib.WARP_F64, xy.ctypes.data, fl.ctypes.data))
    warp = median_ms(export, a.warmup, max(3, a.reps // 3))
    ns = min(a.scatter_events, n)
    vs = [v for v in frames(240, 180) if v.t_lo_ns <= t[ns - 1]]
    t0 = time.perf_counter()
    host_scatter(xy[:ns, 0], xy[:ns, 1], fl[:ns], t[:ns], a.pano, vs, 240, 180)
    scatter_ms = 1e3 * (time.perf_counter() - t0)
    be.reconstruct_end()
    be.close()
    store.close()

    Ls = ["pinhole views of a reconstruction: cmx_backend_recon_view_add_from / _view_get / _view_render",
          "commit %s; %d events over %.0f s from the event store, sensor %dx%d, panorama %dx%d, linear spline of %d knots, batch %d, "
          "default mode" % (commit, n, a.seconds, W, H, Wp, Hp, len(knots), a.batch),
          "host clock around synchronous calls, ms: median (min) of %d after %d warm-up calls, one run" % (a.reps, a.warmup), "",
          "recon_add_from over the %d events (the count panorama), before / after the rows below   %8.3f (%.3f) / %8.3f (%.3f)" %
          ((n,) + add + add_after), "",
          "view_add_from over the same events                  views     size    sets       ms (min)       / add_from    votes counted"]
    for label, nv, Wv, Hv, parts, ms, lo, votes in rows:
        Ls.append("  %-44s   %5d  %4dx%-4d   %3d   %8.3f (%.3f)    %5.2fx    %d" % (label, nv, Wv, Hv, parts, ms, lo, ms / add[0], votes))
    Ls += ["", "one frame out of a voted set                          view_get           view_render"]
    for (Wv, Hv), (g, r) in per_frame.items():
        Ls.append("  %4dx%-4d                                    %8.3f (%.3f)   %8.3f (%.3f)" % ((Wv, Hv) + g + r))
    Ls += ["", "the route these calls replace: per-event export to the host, re-projection and scatter there",
           "  warp_from, fp64 coordinates + flags of all %d events into host arrays                  %8.3f (%.3f)" % ((n,) + warp),
           "  numpy: undo the projection, re-project, scatter the FIRST %d events into %d frames of 240x180, once   %8.1f   "
           "(%.1f s per 20M at that rate)" % (ns, len(vs), scatter_ms, scatter_ms * 20e6 / ns * 1e-3)]
    text = "\n".join(Ls) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
