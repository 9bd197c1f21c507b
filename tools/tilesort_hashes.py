#!/usr/bin/env python3
"""sha256 of contrast, gradient and plane bytes, in deterministic mode, of every path that goes through the tile sort (TileSort,
cmx_tilesort.cpp) -- for comparing two builds of the library on one GPU: run once per build (CMAX_HIP_SO selects the library),
each run a fresh process, and diff the outputs.  Every line must be equal.

  recon     the "window" case of the reconstruction tests (20 000 events, cubic K = 10, batch 100), unbound (reconstruct_eval) and
            bound (reconstruct_bind + reconstruct_eval_bound), on 256 x 128 (counting sort) and on 4128 x 2048 (radix sort)
  backend   one window evaluation, a forced re-sort (prepare), the evaluation again
  frontend  one packet on the production path and on the reference-shaped path

The reference-shaped path never sorts and votes with fp32 atomics in global memory, in an order that varies from run to run --
deterministic mode does not cover it -- so its hashes differ between two runs of ONE library too: its line also carries the
values, to be compared to rounding.

Not a test: it asserts nothing.  Needs a GPU."""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from cmax_slam_amd import _lib, evaluator, synth  # noqa: E402

SENSOR = (240, 180, 200.0, 200.0, 119.5, 89.5)


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()[:32]


def show(tag, contrast, grad, *planes):
    print("%-44s contrast %s  gradient %s  planes %s" % (tag, sha(np.float64(contrast)), sha(grad), " ".join(sha(p) for p in planes)), flush=True)


def recon(Wp, Hp):
    W, H, fx, fy, cx, cy = SENSOR
    order, K, dt = 4, 10, 0.05
    w = synth.backend_window(20_000, W, H, fx, fy, cx, cy, 256, 128, order, K, 0, (K - order + 1) * dt, dt_knots=dt, seed=13, knot_sigma=0.02)
    be = evaluator.BackendEvaluator(W, H, w.lut, Wp, Hp)
    be.set_deterministic(True)
    store = evaluator.EventStore(W, H, len(w.x))
    store.push(w.x, w.y, w.t_ns)
    be.reconstruct_begin(order, w.knots_init, w.start_ns, w.dt_ns, 100, 1)
    c, g = be.reconstruct_eval(store, 0, len(w.x), knots=w.knots_init)
    show("recon %d x %d unbound" % (Wp, Hp), c, g, be.reconstruct_get())
    be.reconstruct_bind(store, 0, len(w.x))
    for i in range(2):
        c, g = be.reconstruct_eval_bound(w.knots_init)
        show("recon %d x %d bound, evaluation %d" % (Wp, Hp, i), c, g, be.reconstruct_get())
    print("    sorts %d" % be.reconstruct_bound_info()["sorts"])
    be.reconstruct_end()
    store.close()


def backend():
    W, H, fx, fy, cx, cy = SENSOR
    w = synth.backend_window(20_000, W, H, fx, fy, cx, cy, 256, 128, 4, 10, 3, 0.35, seed=4)
    be = evaluator.BackendEvaluator(w.W, w.H, w.lut, w.Wp, w.Hp)
    be.set_deterministic(True)
    be.set_window(w.x, w.y, w.t_ns, w.order, w.knots_init, w.start_ns, w.dt_ns, w.num_fixed, w.t_next_win_beg_ns)
    d = np.random.default_rng(1).normal(0, 1e-3, w.P)
    for tag in ("first sort", "after a forced re-sort"):
        c, g = be.eval(d, True)
        show("backend window, " + tag, c, g, be.get_plane(_lib.PLANE_IL_OLD), be.get_plane(_lib.PLANE_IL_NEW))
        be.prepare(d)
    print("    sorts %d" % be.stats()["rebins"])


def frontend():
    p = synth.frontend_packet(50_000, 240, 180, 200.0, 200.0, 119.5, 89.5, seed=3)
    om = (0.3, -0.5, 0.2)
    for path in ("production", "reference-shaped"):
        fe = evaluator.FrontendEvaluator(p.W, p.H, p.lut)
        fe.set_deterministic(True)
        if path == "reference-shaped":
            fe.set_reference_path()
        fe.set_packet(p.x, p.y, p.t_ns, p.t_ref_ns, p.fx, p.fy, p.cx, p.cy, p.batch, p.sigma, 0)
        c, g = fe.eval(om)
        show("frontend packet, %s path" % path, c, g, fe.computeImageOfWarpedEvents(om, blur=False))
        if path == "reference-shaped":
            print("    VALUES contrast %.17g gradient %s" % (c, " ".join("%.17g" % v for v in g)))
        print("    sorts %d" % fe.stats()["rebins"])


if __name__ == "__main__":
    print("library: %s" % os.path.relpath(_lib.SO_PATH, ROOT))
    recon(256, 128)
    recon(4128, 2048)
    backend()
    frontend()
