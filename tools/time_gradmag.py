#!/usr/bin/env python3
"""Sobel gradient-magnitude contrast (contrast_measure = 2): what one evaluation costs on the production path.

Rows, all at BASELINE config 2's shape (1M events, 640x480, sigma = 1), one process, one GPU:

  measure 2, default context           adjoint form: splat, image_adjoint_sobel pass, gather with the finalize as its tail
  measure 2, reference-shaped context  derivative planes, one global atomic per vote, Sobel moments launch, finalize launch
  measure 1, default context           mean-square: the same splat and gather launches around the ordinary image pass

f = cost-only evaluation, fdf = cost and gradient.  Host clock around the synchronous call, the evaluation point alternating
between two points so that no call finds the image of its own point resident.  Median of --reps calls after --warmup warm-up
calls; a second pass with the library's per-class kernel timers on gives the device time per class of one fdf.

Same-box comparison of two builds: run once per library with CMAX_HIP_SO (see tools/ab_builds.sh) and --append; the other
build's library is `make -C cmax_slam_amd/csrc` in a checkout of that commit, copied to tools/ab/.  E.g.
  CMAX_HIP_SO=$PWD/tools/ab/lib_parent.so python tools/time_gradmag.py --label parent
  python tools/time_gradmag.py --label this --append
Writes profiles/gradmag_adjoint.txt.  Needs a GPU; there is no fallback."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from cmax_slam_amd import _lib, evaluator, synth  # noqa: E402


def median_us(call, points, warmup, reps):
    for i in range(warmup):
        call(points[i % 2])
    t = []
    for i in range(reps):
        t0 = time.perf_counter()
        call(points[i % 2])
        t.append((time.perf_counter() - t0) * 1e6)
    return statistics.median(t), min(t)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--events", type=int, default=1_000_000)
    ap.add_argument("--label", default="this build")
    ap.add_argument("--append", action="store_true", help="append to --out instead of replacing it")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gradmag_adjoint.txt"))
    args = ap.parse_args()
    assert _lib.lib().cmx_device_count() > 0, "no GPU visible: this tool measures on the device only"
    try:
        import torch
        box = "%s (%s)" % (torch.cuda.get_device_name(0), torch.cuda.get_device_properties(0).gcnArchName)
    except Exception:
        box = "unknown device"
    p = synth.config2(N=args.events)
    om = np.asarray(p.omega_true, np.float64)
    points = (om, om + np.array([0.01, -0.01, 0.005]))
    rows, classes = [], []
    for name, measure, reference in (("measure 2, default context", 2, False), ("measure 2, reference-shaped context", 2, True),
                                     ("measure 1, default context", 1, False)):
        fe = evaluator.FrontendEvaluator(p.W, p.H, p.lut)
        if reference:
            fe.set_reference_path()
        fe.set_packet(p.x, p.y, p.t_ns, p.t_ref_ns, p.fx, p.fy, p.cx, p.cy, p.batch, p.sigma, measure)
        f_med, f_min = median_us(lambda x: fe.eval(x, False), points, args.warmup, args.reps)
        g_med, g_min = median_us(lambda x: fe.eval(x, True), points, args.warmup, args.reps)
        rows.append((name, f_med, f_min, g_med, g_min))
        fe.timing_enable()
        fe.timing_get()
        for i in range(args.reps):
            fe.eval(points[i % 2], True)
        t = fe.timing_get()
        classes.append((name, {k: (ms * 1e3 / args.reps, n / args.reps) for k, (ms, n) in t.items() if n}))
        fe.close()

    lines = ["== %s ==" % args.label,
             "device: %s    library: %s" % (box, os.path.basename(_lib.SO_PATH)),
             "%d events, %dx%d, sigma %.1f, batch %d; median of %d calls after %d warm-up calls, host clock around the synchronous call" %
             (len(p.x), p.W, p.H, p.sigma, p.batch, args.reps, args.warmup), "",
             "%-38s %12s %12s %12s %12s" % ("row", "f us", "f min us", "fdf us", "fdf min us")]
    for name, f_med, f_min, g_med, g_min in rows:
        lines.append("%-38s %12.1f %12.1f %12.1f %12.1f" % (name, f_med, f_min, g_med, g_min))
    lines += ["", "device time per fdf by kernel class (the library's timers; us per evaluation x launches per evaluation):"]
    for name, t in classes:
        lines.append("%-38s %s" % (name, "  ".join("%s %.1f x%.1f" % (k, us, n) for k, (us, n) in t.items())))
    text = "\n".join(lines) + "\n\n"
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a" if args.append else "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
