#!/usr/bin/env python3
"""Timing of the signed polarity panorama (cmx_backend_recon_pol_*) -> profiles/recon_pol_timing.txt.

tools/time_recon.py's large configuration -- 20M events over 20 s from the event store, 1280x720 sensor, 4096x2048 panorama, linear
spline with 401 knots, batch 100 -- host clock around the synchronous calls, medians of --reps after --warmup, all in one run:
    votes      pol_add_from (ON / OFF planes, the store's polarity bytes) against add_from (the count plane) over the same events,
               in default and in deterministic mode
    render     pol_render (mono8 and bgr8) against recon_render (mono8) of the same panorama size
    the route it replaces   warp_from into host arrays (fp64 coordinates + flags, all events) plus a numpy scatter of the bilinear
               votes into two planes; the scatter is timed on the first --scatter-events events only (it takes seconds at 20M)
Polarities are drawn from a seeded generator: the synthetic stream has none.  Needs a GPU."""
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


def median_ms(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    v = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        v.append(1e3 * (time.perf_counter() - t0))
    return statistics.median(v), min(v)


def host_scatter(xy, fl, pol, Hp, Wp):
    """the bilinear votes of the events with flags == 3 into an ON and an OFF plane, in numpy"""
    planes = np.zeros((2, Hp * Wp), np.float32)
    m = fl == 3
    px, py, off = xy[m, 0], xy[m, 1], (pol[m] == 0).astype(np.int64)
    xx, yy = px.astype(np.int64), py.astype(np.int64)
    dx, dy = (px - xx).astype(np.float32), (py - yy).astype(np.float32)
    one = np.float32(1)
    for w, oy, ox in (((one - dx) * (one - dy), 0, 0), (dx * (one - dy), 0, 1), ((one - dx) * dy, 1, 0), (dx * dy, 1, 1)):
        np.add.at(planes, (off, (yy + oy) * Wp + (xx + ox)), w)
    return planes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--events", type=int, default=20_000_000)
    ap.add_argument("--seconds", type=float, default=20.0)
    ap.add_argument("--sensor", type=int, nargs=2, default=(1280, 720))
    ap.add_argument("--pano", type=int, nargs=2, default=(4096, 2048))
    ap.add_argument("--batch", type=int, default=100)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--scatter-events", type=int, default=1_000_000)
    ap.add_argument("--commit", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "recon_pol_timing.txt"))
    a = ap.parse_args()
    from cmax_slam_amd import _lib, evaluator
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
    pol = np.random.default_rng(7).integers(0, 2, n).astype(np.uint8)
    Wp, Hp = a.pano
    store = evaluator.EventStore(a.sensor[0], a.sensor[1], n)
    store.push(x, y, t, polarity=pol)

    votes = {}
    for mode in ("default", "deterministic"):
        be = evaluator.BackendEvaluator(a.sensor[0], a.sensor[1], lut, Wp, Hp)
        be.set_deterministic(mode == "deterministic")
        be.reconstruct_begin(2, knots, start_ns, dt_ns, a.batch, 1)
        r = {"add": median_ms(lambda: be.reconstruct_add_from(store, 0, n), a.warmup, a.reps),
             "pol": median_ms(lambda: be.reconstruct_pol_add_from(store, 0, n), a.warmup, a.reps)}
        if mode == "default":
            r["add_host"] = median_ms(lambda: be.reconstruct_add(x, y, t), 1, 5)
            r["pol_host"] = median_ms(lambda: be.reconstruct_pol_add(x, y, t, pol), 1, 5)
            # one pass each from here on, so that the renders show a picture and the counts say what voted
            be.reconstruct_restart(knots)
            be.reconstruct_add_from(store, 0, n)
            be.reconstruct_pol_add_from(store, 0, n)
            n_inside = be.reconstruct_get(with_counts=True)[2]
            on, off, n_on, n_off = be.reconstruct_pol_get(with_counts=True)
            assert n_on + n_off == n_inside
            render = {"count": median_ms(lambda: be.reconstruct_render(0.75), a.warmup, a.reps),
                      "mono": median_ms(lambda: be.reconstruct_pol_render(0.75, 0), a.warmup, a.reps),
                      "bgr": median_ms(lambda: be.reconstruct_pol_render(0.75, 1), a.warmup, a.reps)}
            get = {"count": median_ms(lambda: be.reconstruct_get(), a.warmup, a.reps),
                   "pol": median_ms(lambda: be.reconstruct_pol_get(), a.warmup, a.reps)}
            # the route the calls replace: export every event's coordinates to the host, scatter there
            xy, fl = np.zeros((n, 2)), np.zeros(n, np.uint8)  # (touched: no first-touch page faults inside the timed call)

            def export():
                be._ck(L.cmx_backend_recon_warp_from(be._ctx, store._h, 0, n, _lib.WARP_F64, xy.ctypes.data, fl.ctypes.data))
            warp = median_ms(export, a.warmup, a.reps)
            ns = min(a.scatter_events, n)
            t0 = time.perf_counter()
            host = host_scatter(xy[:ns], fl[:ns], pol[:ns], Hp, Wp)
            scatter_ms = 1e3 * (time.perf_counter() - t0)
            del xy, fl, host
        be.reconstruct_end()
        be.close()
        votes[mode] = r
    store.close()

    Ls = ["signed polarity panorama: cmx_backend_recon_pol_add_from / _pol_render",
          "commit %s; %d events over %.0f s from the event store (polarity drawn from a seeded generator), sensor %dx%d, panorama %dx%d, "
          "linear spline of %d knots, batch %d" % (commit, n, a.seconds, a.sensor[0], a.sensor[1], Wp, Hp, len(knots), a.batch),
          "host clock around synchronous calls, ms: median (min) of %d after %d warm-up calls, one run" % (a.reps, a.warmup), "",
          "vote pass over the same %d events              count plane (add_from)      ON / OFF planes (pol_add_from)      pol / count" % n]
    for mode in ("default", "deterministic"):
        r = votes[mode]
        Ls.append("  %-14s                                   %8.3f (%.3f)               %8.3f (%.3f)              %5.2fx" %
                  (mode, r["add"][0], r["add"][1], r["pol"][0], r["pol"][1], r["pol"][0] / r["add"][0]))
    r = votes["default"]
    Ls += ["  from host arrays, default (median of 5)          %8.3f (%.3f)               %8.3f (%.3f)              %5.2fx" %
           (r["add_host"][0], r["add_host"][1], r["pol_host"][0], r["pol_host"][1], r["pol_host"][0] / r["add_host"][0]),
           "  %d ON + %d OFF events voted = the %d of add_from" % (n_on, n_off, n_inside), "",
           "tone map of the %dx%d panorama, device pass + pinned copy + copy to the caller" % (Wp, Hp),
           "  recon_render mono8 (count plane)     %8.3f (%.3f)" % render["count"],
           "  pol_render mono8 (ON - OFF)          %8.3f (%.3f)      %5.2fx" % (render["mono"] + (render["mono"][0] / render["count"][0],)),
           "  pol_render bgr8  (ON - OFF)          %8.3f (%.3f)      %5.2fx  (three times the bytes)" %
           (render["bgr"] + (render["bgr"][0] / render["count"][0],)),
           "  recon_get (one fp32 plane)           %8.3f (%.3f)" % get["count"],
           "  pol_get (two fp32 planes)            %8.3f (%.3f)" % get["pol"], "",
           "the route these calls replace: per-event export to the host, scatter there",
           "  warp_from, fp64 coordinates + flags of all %d events into host arrays     %8.3f (%.3f)" % ((n,) + warp),
           "  numpy scatter of the votes of the FIRST %d events into two planes, once   %8.1f   (%.1f s per 20M at that rate)" %
           (ns, scatter_ms, scatter_ms * 20e6 / ns * 1e-3),
           "  pol_add_from over all %d events                                           %8.3f" % (n, r["pol"][0])]
    text = "\n".join(Ls) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
