#!/usr/bin/env python3
"""Timing of the per-event support scores (cmx_backend_recon_score*) -> profiles/recon_score_timing.txt.

tools/time_recon.py's large configuration -- 20M events over 20 s from the event store, 1280x720 sensor, 4096x2048 panorama, linear
spline with 401 knots, batch 100 -- host clock around the synchronous calls, medians of --reps after --warmup, all in ONE run:
    score_open            sigma 0 (the plane itself) and sigma 1 (tile flags, memset, the smoothing pass over the occupied tiles)
    score_from_device     scores + flags into device tensors, leave-one-out on and off, at both sigmas
    score_from            into host arrays the host has touched before
    beside them           warp_from_device (fp32 coordinates + flags) and add_from's vote pass over the same events
--device-only skips the host-output part (comparing two builds of the kernel: CMAX_HIP_SO selects the library, --label names it,
--append adds the table to the file instead of replacing it).  Needs a GPU."""
import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402

import time_recon as tr  # noqa: E402  (the stream of the large configuration)
from time_recon_warp import median_ms  # noqa: E402


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
    ap.add_argument("--append", action="store_true")
    ap.add_argument("--label", default="")
    ap.add_argument("--commit", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "recon_score_timing.txt"))
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
    d_fl = torch.empty(n, dtype=torch.uint8, device="cuda")
    d_xy = torch.empty((n, 2), dtype=torch.float32, device="cuda")
    d_sc = torch.empty(n, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    warp = median_ms(lambda: be.reconstruct_warp_from(store, 0, n, dtype=np.float32, out=(d_xy, d_fl)), a.warmup, a.reps)
    del d_xy
    rows = []
    for sigma in (0.0, 1.0):
        r = {"sigma": sigma}
        r["open"] = median_ms(lambda: be.reconstruct_score_open(sigma), a.warmup, a.reps)
        r["loo"] = median_ms(lambda: be.reconstruct_score_from(store, 0, n, loo=True, out=(d_sc, d_fl)), a.warmup, a.reps)
        r["plain"] = median_ms(lambda: be.reconstruct_score_from(store, 0, n, loo=False, out=(d_sc, d_fl)), a.warmup, a.reps)
        r["noflags"] = median_ms(lambda: be.reconstruct_score_from(store, 0, n, loo=True, out=(d_sc, None)), a.warmup, a.reps)
        if not a.device_only:
            sc, fl = np.zeros(n, np.float32), np.zeros(n, np.uint8)  # (touched: no first-touch page faults inside the timed call)

            def host():
                be._ck(L.cmx_backend_recon_score_from(be._ctx, store._h, 0, n, 1, sc.ctypes.data, fl.ctypes.data))
            r["host"] = median_ms(host, a.warmup, a.reps)
            r["mean"] = float(sc.mean(dtype=np.float64))
            r["below1"] = float(np.mean(sc[fl == 3] < 1.0))
            del sc, fl
        rows.append(r)
    be.reconstruct_end()
    store.close()

    Ls = ["per-event support scores: cmx_backend_recon_score_open / _score_from_device / _score_from%s" % ((" [" + a.label + "]") if a.label else ""),
          "commit %s; %d events over %.0f s from the event store, sensor %dx%d, panorama %dx%d, linear spline of %d knots, batch %d" %
          (commit, n, a.seconds, a.sensor[0], a.sensor[1], a.pano[0], a.pano[1], len(knots), a.batch),
          "host clock around synchronous calls, ms: median (min) of %d after %d warm-up calls; the plane holds %d vote passes" %
          (a.reps, a.warmup, a.reps + a.warmup), "",
          "vote pass over the same events, same run (add_from)                      %8.3f (%.3f)" % votes,
          "export, fp32 coordinates + flags, same run (warp_from_device)            %8.3f (%.3f)" % warp, "",
          "sigma   score_open           score_from_device: loo + flags      no loo + flags       loo, no flags        vs export   vs votes"]
    for r in rows:
        Ls.append("  %-3g   %8.3f (%.3f)    %8.3f (%.3f)                  %8.3f (%.3f)   %8.3f (%.3f)      %5.2fx     %5.2fx" %
                  (r["sigma"], r["open"][0], r["open"][1], r["loo"][0], r["loo"][1], r["plain"][0], r["plain"][1], r["noflags"][0],
                   r["noflags"][1], r["loo"][0] / warp[0], r["loo"][0] / votes[0]))
    if not a.device_only:
        Ls += ["", "host output (score_from, loo, into touched host arrays; 5 bytes per event)      call      mean score      voting events below one vote"]
        for r in rows:
            Ls.append("  sigma %-3g                                                              %8.3f (%.3f)   %10.3f      %5.1f %%" %
                      (r["sigma"], r["host"][0], r["host"][1], r["mean"], 100.0 * r["below1"]))
    text = "\n".join(Ls) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a" if a.append else "w") as f:
        if a.append:
            f.write("\n")
        f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
