#!/usr/bin/env python3
"""sha256 of what the three target sets of a reconstruction hold -- the planes of the pinhole views, the volumes of the voxel grids,
the cells of the time surfaces, and every n_voted counter -- after one pass over a whole stream through each of add, add_aos and
add_from: for comparing two builds of the library on one GPU.  Run once per build (CMAX_HIP_SO selects the library), each run a
fresh process, and diff the outputs: they must be identical.  Modelled on tools/image_pass_hashes.py.

Views and voxel grids are hashed in DETERMINISTIC mode, where a cell is a sum of integers and does not depend on the order of the
atomics; a surface cell is a maximum of integers and is hashed in both modes.  The sets are those of tests/recon_view_cases.py,
tests/recon_voxel_cases.py and tests/recon_surface_cases.py, all of them: a partial last run (n65), more matching targets than an
LDS chunk holds (overlap40, stack10, overlap10), a batch that spans several targets (batch5000), rays behind the camera and off the
plane (poles, behind), signed and unsigned voxel sets and by-polarity and merged surface sets (one_bin is the unsigned / merged
one), spline orders 2 (linear, B2) and 4.

Not a test: it asserts nothing.  Needs a GPU."""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402

import recon_cases as rc  # noqa: E402
import recon_pol_cases as pc  # noqa: E402
import recon_surface_cases as sc  # noqa: E402
import recon_view_cases as vc  # noqa: E402
import recon_voxel_cases as xc  # noqa: E402
from cmax_slam_amd import _lib, evaluator as hip, trajectory  # noqa: E402

W, H = rc.SENSOR[:2]


class po:
    """What the case modules ask of the checker they are handed -- the spline's pose at a time -- from the library's own host
    evaluation (cmx_traj_evaluate): a tool does not load the checker, and both builds are given the same sets either way."""

    @staticmethod
    def spline_eval(order, knots, start_ns, dt_ns, t_ns, jac=False):
        k, q = np.ascontiguousarray(knots, np.float64).reshape(-1, 4), np.zeros(4)
        trajectory._chk(_lib.lib().cmx_traj_evaluate(int(order), len(k), trajectory._d(k), int(start_ns), int(dt_ns), int(t_ns),
                                                     trajectory._d(q)), "cmx_traj_evaluate")
        return (q,)


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()[:32]


def run(kind, name, case, deterministic, begin, add, add_aos, add_from, get, end, with_pol):
    """one evaluator per ingest path: begin the set, one pass over the whole stream, hash what the set holds"""
    c, (w, x, y, t) = rc.CASES[case], rc.window(case)
    pol = pc.polarity(case)
    for path in ("add", "add_aos", "add_from"):
        be = hip.BackendEvaluator(W, H, w.lut, c["Wp"], c["Hp"])
        be.set_deterministic(deterministic)
        be.reconstruct_begin(c["order"], w.knots_true, w.start_ns, w.dt_ns, c["batch"], c["rate"])
        begin(be)
        tag = "%-8s %-20s order %d %-13s %-8s" % (kind, name, c["order"], "deterministic" if deterministic else "default", path)
        try:
            if path == "add":
                add(be, x, y, t, pol)
            elif path == "add_aos":
                add_aos(be, _lib.dvs_events(x, y, t, pol))
            else:
                store = hip.EventStore(W, H, max(len(x), 1))
                if len(x):
                    store.push(x, y, t, polarity=pol if with_pol else None)
                add_from(be, store, 0, len(x))
                store.close()
            cells, counts = get(be)
            print("%s cells %s  n_voted %s  (%d voted)" % (tag, sha(cells), sha(counts), int(counts.sum())), flush=True)
        except _lib.CmaxHipError as e:  # (an input a path refuses is refused by both builds, in the same words)
            print("%s refused: %s" % (tag, e), flush=True)
        end(be)
        be.reconstruct_end()
        be.close()


def views(name):
    case, Wv, Hv, vs = vc.view_set(po, name)
    run("view", name, case, True, lambda be: be.reconstruct_view_begin(vs, Wv, Hv),
        lambda be, x, y, t, pol: be.reconstruct_view_add(x, y, t), lambda be, ev: be.reconstruct_view_add_aos(ev),
        lambda be, *a: be.reconstruct_view_add_from(*a), lambda be: be.reconstruct_view_get(with_counts=True),
        lambda be: be.reconstruct_view_end(), False)


def voxels(name):
    case, Wv, Hv, n_bins, signed, grids = xc.voxel_set(po, name)
    run("voxel", "%s%s" % (name, "" if signed else " (unsigned)"), case, True, lambda be: be.reconstruct_voxel_begin(grids, Wv, Hv, n_bins, signed),
        lambda be, x, y, t, pol: be.reconstruct_voxel_add(x, y, t, pol), lambda be, ev: be.reconstruct_voxel_add_aos(ev),
        lambda be, *a: be.reconstruct_voxel_add_from(*a), lambda be: be.reconstruct_voxel_get(with_counts=True),
        lambda be: be.reconstruct_voxel_end(), True)


def surfaces(name, deterministic):
    case, Wv, Hv, by_pol, ss = sc.surface_set(po, name)
    run("surface", "%s%s" % (name, "" if by_pol else " (merged)"), case, deterministic, lambda be: be.reconstruct_surface_begin(ss, Wv, Hv, by_pol),
        lambda be, x, y, t, pol: be.reconstruct_surface_add(x, y, t, pol), lambda be, ev: be.reconstruct_surface_add_aos(ev),
        lambda be, *a: be.reconstruct_surface_add_from(*a), lambda be: be.reconstruct_surface_get(with_counts=True),
        lambda be: be.reconstruct_surface_end(), True)


if __name__ == "__main__":
    print("library: %s" % os.path.relpath(_lib.SO_PATH, ROOT))
    for name in vc.SETS:
        views(name)
    for name in xc.SETS:
        voxels(name)
    for name in sc.SETS:
        for det in (True, False):
            surfaces(name, det)
