#!/usr/bin/env python3
"""Timing of the per-event export (cmx_backend_recon_warp*) -> profiles/recon_warp_timing.txt.

tools/time_recon.py's large configuration -- 20M events over 20 s from the event store, 1280x720 sensor, 4096x2048 panorama, linear
spline with 401 knots, batch 100 -- host clock around the synchronous calls, medians of --reps after --warmup:
    device output   warp_from_device in both formats (coordinates + flags into device tensors), against add_from's vote pass over the
                    same events in the same run
    host output     warp_from in both formats into arrays the host has touched before, against a plain pinned device-to-host
                    copy of the same byte count; the copy's share of the call
--device-only skips the host-output part (comparing two builds of the kernel: CMAX_HIP_SO selects the library).  Needs a GPU."""
import argparse
import ctypes as C
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--events", type=int, default=20_000_000)
    ap.add_argument("--seconds", type=float, default=20.0)
    ap.add_argument("--sensor", type=int, nargs=2, default=(1280, 720))
    ap.add_argument("--pano", type=int, nargs=2, default=(4096, 2048))
    ap.add_argument("--batch", type=int, default=100)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--device-only", action="store_true")
    ap.add_argument("--label", default="")
    ap.add_argument("--commit", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "recon_warp_timing.txt"))
    a = ap.parse_args()
    import torch
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
    be = evaluator.BackendEvaluator(a.sensor[0], a.sensor[1], lut, a.pano[0], a.pano[1])
    store = evaluator.EventStore(a.sensor[0], a.sensor[1], n)
    store.push(x, y, t)
    be.reconstruct_begin(2, knots, start_ns, dt_ns, a.batch, 1)

    votes = median_ms(lambda: be.reconstruct_add_from(store, 0, n), a.warmup, a.reps)
    rows = []
    d_fl = torch.empty(n, dtype=torch.uint8, device="cuda")
    for name, fmt, tdt, ndt in (("fp64", _lib.WARP_F64, torch.float64, np.float64), ("fp32", _lib.WARP_F32, torch.float32, np.float32)):
        pair = 2 * np.dtype(ndt).itemsize
        d_xy = torch.empty((n, 2), dtype=tdt, device="cuda")
        torch.cuda.synchronize()
        r = {"name": name, "bytes": n * (pair + 1)}
        r["dev"] = median_ms(lambda: be.reconstruct_warp_from(store, 0, n, dtype=ndt, out=(d_xy, d_fl)), a.warmup, a.reps)
        r["dev_noflags"] = median_ms(lambda: be.reconstruct_warp_from(store, 0, n, dtype=ndt, out=(d_xy, None)), a.warmup, a.reps)
        if not a.device_only:
            xy, fl = np.zeros((n, 2), ndt), np.zeros(n, np.uint8)  # (touched: no first-touch page faults inside the timed call)

            def host():
                be._ck(L.cmx_backend_recon_warp_from(be._ctx, store._h, 0, n, fmt, xy.ctypes.data, fl.ctypes.data))
            r["host"] = median_ms(host, a.warmup, a.reps)
            pinned = torch.empty(n * (pair + 1), dtype=torch.uint8).pin_memory()
            dev = torch.empty(n * (pair + 1), dtype=torch.uint8, device="cuda")

            def copy():
                pinned.copy_(dev, non_blocking=True)
                torch.cuda.synchronize()
            r["copy"] = median_ms(copy, a.warmup, a.reps)
            del pinned, dev, xy, fl
        del d_xy
        rows.append(r)
    be.reconstruct_end()
    store.close()

    Ls = ["per-event export: cmx_backend_recon_warp_from_device / _from%s" % ((" [" + a.label + "]") if a.label else ""),
          "commit %s; %d events over %.0f s from the event store, sensor %dx%d, panorama %dx%d, linear spline of %d knots, batch %d" %
          (commit, n, a.seconds, a.sensor[0], a.sensor[1], a.pano[0], a.pano[1], len(knots), a.batch),
          "host clock around synchronous calls, ms: median (min) of %d after %d warm-up calls" % (a.reps, a.warmup), "",
          "vote pass over the same events, same run (add_from, unchanged code)      %8.3f (%.3f)" % votes, "",
          "device output (warp_from_device)      coordinates + flags      coordinates only      bytes written      GB/s      vs votes"]
    for r in rows:
        Ls.append("  %-6s                          %8.3f (%.3f)      %8.3f (%.3f)     %12d   %8.1f      %5.2fx" %
                  (r["name"], r["dev"][0], r["dev"][1], r["dev_noflags"][0], r["dev_noflags"][1], r["bytes"],
                   1e-6 * r["bytes"] / r["dev"][0], r["dev"][0] / votes[0]))
    if not a.device_only:
        Ls += ["", "host output (warp_from into touched host arrays)      call      plain pinned D2H copy of the same bytes      copy / call"]
        for r in rows:
            Ls.append("  %-6s                                      %8.3f (%.3f)      %8.3f (%.3f)  %6.1f GB/s               %5.1f%%" %
                      (r["name"], r["host"][0], r["host"][1], r["copy"][0], r["copy"][1], 1e-6 * r["bytes"] / r["copy"][0],
                       100.0 * r["copy"][0] / r["host"][0]))
    text = "\n".join(Ls) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
