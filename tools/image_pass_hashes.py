#!/usr/bin/env python3
"""sha256 of contrast, gradient and Jt bytes of every form of the image kernels in cmx_kernels.hip (image_moments,
image_adjoint_kernel, image_adjoint2<4>, image_adjoint2g, image_adjoint_sobel and their tile-list variants) -- for comparing two
builds of the library on one GPU: run once per build (CMAX_HIP_SO selects the library), each run a fresh process, and diff the
outputs.  Modelled on tools/tilesort_hashes.py.

Front-end inputs are tests/dense_image_ops.exact_packet at omega = 0 (integer-pixel events: the forward plane is an exact count per
pixel whatever the order of the atomics); the window and reconstruction cases are those of tests/test_gpu_adjoint_plane.py.  Sizes
are the smallest at which each form exists and its partial-tile and border code runs.  Jt is hashed over
dense_image_ops.compare_set only: the tiles outside it keep whatever an earlier pass left.

Lines marked VALUES vary from run to run of ONE library and are compared to rounding (1e-12 relative), not by hash:
  * the device-driven solve (TAIL 2 / TAIL 3 of image_adjoint2<4>): TAIL 3 sums the tile moments with fp64 atomics in arrival order,
    and deterministic mode does not chain;
  * the 2048 x 1056 window with a tile list: deterministic mode takes no list, so the votes are fp32 atomics and the list is in
    arrival order.  (The same window is also run in deterministic mode, without a list, and the reconstruction's list form is
    deterministic.)
  * the derivative-plane gradient (GRAD_PLANES): one global fp32 atomic per derivative vote.

Not a test: it asserts nothing.  Needs a GPU."""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402

import adjoint_forms as af  # noqa: E402
import dense_image_ops as dio  # noqa: E402
import recon_cases as rc  # noqa: E402
import recon_grad_cases as rg  # noqa: E402
from cmax_slam_amd import _lib, evaluator, synth  # noqa: E402


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()[:32]


def show(tag, contrast, grad, jt=None, mask=None, values=False):
    g = np.zeros(0) if grad is None else np.asarray(grad, np.float64)
    print("%-66s contrast %s  gradient %s  Jt %s" % (tag, sha(np.float64(contrast)), sha(g), sha(jt[mask]) if jt is not None else "-"), flush=True)
    if values:
        print("    VALUES contrast %.17g gradient %s" % (contrast, " ".join("%.17g" % v for v in g)))


def frontend(tag, W, H, sigma, measure=0, options=(), script="fdf", planes=False):
    p = dio.exact_packet(W, H)
    A = dio.exact_counts(p)
    fe = evaluator.FrontendEvaluator(p.W, p.H, p.lut)
    fe.set_deterministic(True)
    if planes:
        fe.set_grad_mode(_lib.GRAD_PLANES)
    for key, value in options:
        fe.set_option(getattr(_lib, "OPT_" + key), value)
    fe.set_packet(p.x, p.y, p.t_ns, p.t_ref_ns, p.fx, p.fy, p.cx, p.cy, p.batch, sigma, measure)
    mask = dio.compare_set(A, dio.radius(sigma), dio.jt_reach(sigma, measure))
    tag = "%s %dx%d sigma %g" % (tag, W, H, sigma)
    if script == "f_df":  # a cost-only evaluation (finalize in the image pass's tail), then the df that reuses its Jt
        c, _ = fe.eval(np.zeros(3), want_grad=False)
        show(tag + ", f", c, None, None if planes else fe.adjoint_plane(), mask)
    if script == "f":
        c, _ = fe.eval(np.zeros(3), want_grad=False)
        show(tag + ", f", c, None)
    else:
        c, g = fe.eval(np.zeros(3))
        show(tag + (", df" if script == "f_df" else ", fdf"), c, g, None if planes else fe.adjoint_plane(), mask, values=planes)
    fe.close()


def window(tag, w, sigma, det):
    be = evaluator.BackendEvaluator(w.W, w.H, w.lut, w.Wp, w.Hp)
    if det:
        be.set_deterministic(True)
    be.set_window(w.x, w.y, w.t_ns, w.order, w.knots_init, w.start_ns, w.dt_ns, w.num_fixed, w.t_next_win_beg_ns, w.batch, w.sample_rate,
                  sigma, _lib.VARIANCE, None)
    c, g = be.eval(0.01 * np.cos(np.arange(w.P)))
    A = be.get_plane(_lib.PLANE_IL_OLD) + be.get_plane(_lib.PLANE_IL_NEW)
    show("%s %dx%d sigma %g%s" % (tag, w.Wp, w.Hp, sigma, ", deterministic" if det else ""), c, g, be.adjoint_plane(),
         dio.compare_set(A, dio.radius(sigma)), values=not det)
    be.close()


def reconstruction(name, sigma):
    if name == "big":
        w = af.be_window("big")
        be = evaluator.BackendEvaluator(w.W, w.H, w.lut, w.Wp, w.Hp)
        be.set_deterministic(True)
        be.reconstruct_begin(w.order, w.knots_init, w.start_ns, w.dt_ns, w.batch, w.sample_rate)
        x, y, t = w.x, w.y, w.t_ns
    else:
        c, (w, x, y, t) = rc.CASES[name], rc.window(name)
        be = evaluator.BackendEvaluator(rc.SENSOR[0], rc.SENSOR[1], w.lut, c["Wp"], c["Hp"])
        be.set_deterministic(True)
        be.reconstruct_begin(c["order"], rg.point(name), w.start_ns, w.dt_ns, c["batch"], c["rate"])
    be.reconstruct_add(x, y, t)
    A = be.reconstruct_get()
    for measure in (0, 1):
        con = be.reconstruct_contrast(sigma, measure, want_grad=True)
        show("reconstruction %s %dx%d sigma %g measure %d" % (name, A.shape[1], A.shape[0], sigma, measure), con, None,
             be.reconstruct_adjoint_plane(), dio.compare_set(A, dio.radius(sigma)))
    be.close()


def chain_solve():
    p = synth.frontend_packet(30_000, 100, 70, 90.0, 90.0, 49.5, 34.5, seed=77)
    for mode in (1, 4):  # 1: self-gating slots (TAIL 3 image passes); 4: finalize behind the image pass (TAIL 2)
        fe = evaluator.FrontendEvaluator(p.W, p.H, p.lut)
        fe.set_fast_path()
        fe.set_option(_lib.OPT_FUSED_IMAGE, 0)
        fe.set_option(_lib.OPT_CHAIN_SOLVE, mode)
        fe.set_packet(p.x, p.y, p.t_ns, p.t_ref_ns, p.fx, p.fy, p.cx, p.cy, p.batch, p.sigma, _lib.VARIANCE)
        x, rep = fe.setupProblemAndOptimize(np.zeros(3))
        st = fe.stats()
        show("device-driven solve, CHAIN_SOLVE %d, 100x70" % mode, rep["final_cost"], x)
        print("    VALUES initial_cost %.17g final_cost %.17g x %s  chain_solves %d takeovers %d slots %d" % (
            rep["initial_cost"], rep["final_cost"], " ".join("%.17g" % v for v in x), st["chain_solves"], st["chain_takeovers"], st["chain_slots"]))
        fe.close()


if __name__ == "__main__":
    print("library: %s" % os.path.relpath(_lib.SO_PATH, ROOT))
    four = (("FUSED_IMAGE", 0), ("COMPOSITE_IMAGE", 0))
    for W, H in [(10, 10), (65, 17), (100, 70)]:
        frontend("four-pass<4> (COMPOSITE_IMAGE 0)", W, H, 1.0, options=four)
    for W, H in [(18, 18), (100, 70)]:
        frontend("four-pass<-1> (COMPOSITE_IMAGE 0)", W, H, 2.0, options=four)
    for W, H in [(65, 17), (128, 32), (100, 70)]:
        frontend("image_adjoint2<4> TAIL 0", W, H, 1.0, options=(("FUSED_IMAGE", 0),))
        frontend("image_adjoint2<4> TAIL 1", W, H, 1.0, options=(("FUSED_IMAGE", 0),), script="f_df")
    for W, H in [(33, 33), (100, 70)]:
        frontend("image_adjoint2g", W, H, 2.0)
    for W, H in [(10, 10), (65, 17), (100, 70)]:
        frontend("image_adjoint_sobel<4>", W, H, 1.0, measure=_lib.GRADIENT_MAGNITUDE)
    frontend("image_adjoint_sobel<-1>", 100, 70, 2.0, measure=_lib.GRADIENT_MAGNITUDE)
    for W, H in [(65, 17), (100, 70)]:
        for sigma in (1.0, 2.0):
            frontend("image_moments (GRAD_PLANES)", W, H, sigma, planes=True)
            frontend("image_moments (GRAD_PLANES)", W, H, sigma, planes=True, script="f")
    window("window", rc.window("window")[0], 1.0, det=True)
    for sigma in (1.0, 1.7):
        window("window (no list)", af.be_window("big"), sigma, det=True)
        window("window, tile list", af.be_window("big"), sigma, det=False)
    reconstruction("pano130x96", 1.0)
    reconstruction("pano130x96", 2.0)
    reconstruction("big", 1.0)
    chain_solve()
