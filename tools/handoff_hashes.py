#!/usr/bin/env python3
"""sha256 of contrast and gradient of every form that runs the device hand-off code (agent-scope accessors, wave and block sums, the
last-arriver ticket, the result publication, column sums to accumulator rows, the bounded polls: cmx_kernels.hip, cmx_fusedgather.hpp,
cmx_selfserve.hpp, cmx_tilepass.hpp) or the gradient vote and its run sum (cmx_warp.hpp) -- for comparing two builds of the library on
one GPU: run once per build (CMAX_HIP_SO selects the library), each run a fresh process, and diff the outputs.  Modelled on
tools/image_pass_hashes.py.

  * the front end with CMX_OPT_FUSED_IMAGE 0 / 1 / 2 / 3 x CMX_OPT_TAIL_FINALIZE 0 / 1 / 2 / 4 (tests/gather_cases.py: the border-band
    packet, 257 and 65 537 events), and TAIL 0 / 1 / 2 / 4 in deterministic mode;
  * a device-driven solve (tools/image_pass_hashes.py: chain_solve);
  * the back end with CMX_OPT_FOLD_BATCH 0 / 1 at orders 2 and 4, per_batch a multiple of four (o2_b28, o4_b88: four events per lane)
    and not (o2_b63, o4_b65: one per lane), as it is and in deterministic mode;
  * the reconstruction gradient (tests/recon_grad_cases.py) in both forms of recon_gather_kernel (DET false / true).

Lines of deterministic mode must be equal between two builds.  Every other form adds fp64 sums (and, back end, fp32 votes) with
atomics in arrival order: its lines are marked VALUES, vary from run to run of ONE library and are compared to rounding (1e-12
relative for the front end, whose vote plane is exact integer arithmetic), not by hash.

Not a test: it asserts nothing.  Needs a GPU."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]
import numpy as np  # noqa: E402

import gather_cases as gc  # noqa: E402
import recon_cases as rc  # noqa: E402
import recon_grad_cases as rg  # noqa: E402
from cmax_slam_amd import _lib, evaluator  # noqa: E402
from image_pass_hashes import chain_solve, show  # noqa: E402


def frontend(tag, p, omega, det, options):
    fe = evaluator.FrontendEvaluator(p.W, p.H, p.lut)
    if det:
        fe.set_deterministic(True)
    for key, value in options:
        fe.set_option(getattr(_lib, "OPT_" + key), value)
    fe.set_packet(p.x, p.y, p.t_ns, p.t_ref_ns, p.fx, p.fy, p.cx, p.cy, p.batch, 1.0, _lib.VARIANCE)
    c, g = fe.eval(np.asarray(omega, np.float64))
    c2, g2 = fe.eval(np.asarray(omega, np.float64))  # once more: the counters and accumulator rows the first one left behind
    st = fe.stats()
    name = "front end %s %s%s" % (tag, " ".join("%s %d" % kv for kv in options), ", deterministic" if det else "")
    show(name, c, g, values=not det)
    show(name + ", again", c2, g2, values=not det)
    print("    fused_evals %d fused_redos %d host_finalize_evals %d" % (st["fused_evals"], st["fused_redos"], st.get("host_finalize_evals", 0)))
    fe.close()


def backend(name, fold, det):
    c, x, y, t, lut, knots, start_ns, dt_ns, _, IG, side = gc.be_case("window", name)
    be = evaluator.BackendEvaluator(gc.SENSOR[0], gc.SENSOR[1], lut, c["Wp"], c["Hp"])
    if det:
        be.set_deterministic(True)
    be.set_option(_lib.OPT_FOLD_BATCH, fold)
    be.set_window(x, y, t, c["order"], knots, start_ns, dt_ns, c["nf"], side, c["per_batch"], c["rate"], c["sigma"], c["measure"], IG)
    con, g = be.eval(gc.be_point("window", name))
    show("back end %s FOLD_BATCH %d%s" % (name, fold, ", deterministic" if det else ""), con, g, values=not det)
    be.close()


def recon_gradient(name, det):
    c, (w, x, y, t) = rc.CASES[name], rc.window(name)
    be = evaluator.BackendEvaluator(rc.SENSOR[0], rc.SENSOR[1], w.lut, c["Wp"], c["Hp"])
    if det:
        be.set_deterministic(True)
    be.reconstruct_begin(c["order"], rg.point(name), w.start_ns, w.dt_ns, c["batch"], c["rate"])
    be.reconstruct_add(x, y, t)
    con = be.reconstruct_contrast(1.0, 0, True)
    be.reconstruct_grad_add(x, y, t)
    g = be.reconstruct_grad_get()
    be.reconstruct_end()
    show("reconstruction gradient %s%s" % (name, ", deterministic" if det else ""), con, g, values=not det)
    be.close()


if __name__ == "__main__":
    print("library: %s" % os.path.relpath(_lib.SO_PATH, ROOT))
    packets = (("band", gc.fe_packet("band", 1.0)), ("257 events", gc.fe_packet("count", 1.0, 257)),
               ("65537 events", gc.fe_packet("count", 1.0, 65_537)))
    for tag, p in packets:
        for tail in (0, 1, 2, 4):
            frontend(tag, p, gc.FE_OMEGAS[1], True, (("TAIL_FINALIZE", tail),))
        for fused in (0, 1, 2, 3):
            for tail in (0, 1, 2, 4):
                frontend(tag, p, gc.FE_OMEGAS[1], False, (("FUSED_IMAGE", fused), ("TAIL_FINALIZE", tail)))
    chain_solve()
    for name in ("o2_b28", "o2_b63", "o4_b88", "o4_b65"):
        for det in (True, False):
            for fold in (0, 1):
                backend(name, fold, det)
    for name in ("pano130x96", "shortest4"):
        for det in (True, False):
            recon_gradient(name, det)
