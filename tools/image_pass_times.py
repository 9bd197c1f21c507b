#!/usr/bin/env python3
"""Device time of the image pass, per form of the image kernels of cmx_kernels.hip, through the library's per-class timers
(timing_enable / timing_get: HIP events around the launches; `image` is the image pass with its tile-list pre-pass).  One line per
form: the classes of an fdf evaluation (and of a cost-only one where that takes another kernel), mean over --reps evaluations after
--warmup, CMX_OPT_REUSE_IMAGE 0 so that every evaluation runs its image pass.

  front end, BASELINE config 2 (1M events, 640 x 480):
    four-pass<4>   (FUSED_IMAGE 0, COMPOSITE_IMAGE 0)     four-pass<-1>  (sigma 2, COMPOSITE_IMAGE 0)
    adjoint2<4>    (FUSED_IMAGE 0; f: its tail form)      adjoint2g      (sigma 2)
    sobel<4>, sobel<-1> (measure 2, sigma 1 and 2)        moments        (GRAD_PLANES: fdf and f)
  back end: the 2048 x 1056 window of tests/adjoint_forms.py (2112 tiles: image_adjoint2<4, true, 0 | 1> over a tile list)

For a same-box comparison of two builds run it once per library, alternating (CMAX_HIP_SO selects one per process; see
tools/ab_builds.sh).  Needs a GPU; asserts nothing."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
os.environ.setdefault("CMAX_HIP_NO_TORCH", "1")
import numpy as np  # noqa: E402

import adjoint_forms as af  # noqa: E402
from cmax_slam_amd import _lib, evaluator, synth  # noqa: E402


def classes(ev, x, want_grad, warmup, reps):
    for _ in range(warmup):
        ev.eval(x, want_grad)
    ev.timing_enable(True)
    ev.timing_get()
    for _ in range(reps):
        ev.eval(x, want_grad)
    t = ev.timing_get()
    ev.timing_enable(False)
    return " ".join("%s=%.2f" % (k, 1e3 * v[0] / v[1]) for k, v in t.items() if v[1])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--only", default="", help="run only the forms whose name contains this (e.g. 'tile list', 'sobel')")
    args = ap.parse_args()
    tag = os.path.basename(_lib.SO_PATH)
    p = synth.config2()
    om = np.array([0.3, -0.5, 0.2])
    forms = (("four-pass<4>", 1.0, 0, (("FUSED_IMAGE", 0), ("COMPOSITE_IMAGE", 0)), False),
             ("four-pass<-1> sigma 2", 2.0, 0, (("COMPOSITE_IMAGE", 0),), False),
             ("adjoint2<4>", 1.0, 0, (("FUSED_IMAGE", 0),), True),
             ("adjoint2g sigma 2", 2.0, 0, (), False),
             ("sobel<4>", 1.0, _lib.GRADIENT_MAGNITUDE, (), False),
             ("sobel<-1> sigma 2", 2.0, _lib.GRADIENT_MAGNITUDE, (), False),
             ("moments (GRAD_PLANES)", 1.0, 0, "planes", True))
    for name, sigma, measure, opts, cost_only in forms:
        if args.only not in name:
            continue
        fe = evaluator.FrontendEvaluator(p.W, p.H, p.lut)
        if opts == "planes":
            fe.set_grad_mode(_lib.GRAD_PLANES)
        else:
            for k, v in opts:
                fe.set_option(getattr(_lib, "OPT_" + k), v)
        fe.set_option(_lib.OPT_REUSE_IMAGE, 0)
        fe.set_packet(p.x, p.y, p.t_ns, p.t_ref_ns, p.fx, p.fy, p.cx, p.cy, p.batch, sigma, measure)
        line = "%s fe 640x480 %-24s fdf us: %s" % (tag, name, classes(fe, om, True, args.warmup, args.reps))
        if cost_only:
            line += " | f us: %s" % classes(fe, om, False, args.warmup, args.reps)
        print(line, flush=True)
        fe.close()
    if args.only not in "tile list":
        return
    w = af.be_window("big")
    be = evaluator.BackendEvaluator(w.W, w.H, w.lut, w.Wp, w.Hp)
    be.set_window(w.x, w.y, w.t_ns, w.order, w.knots_init, w.start_ns, w.dt_ns, w.num_fixed, w.t_next_win_beg_ns, w.batch, w.sample_rate,
                  1.0, _lib.VARIANCE, None)
    be.set_option(_lib.OPT_REUSE_IMAGE, 0)
    x = 0.01 * np.cos(np.arange(w.P))
    print("%s be 2048x1056 tile list          fdf us: %s | f us: %s" % (tag, classes(be, x, True, args.warmup, args.reps),
                                                                        classes(be, x, False, args.warmup, args.reps)), flush=True)
    be.close()


if __name__ == "__main__":
    main()
