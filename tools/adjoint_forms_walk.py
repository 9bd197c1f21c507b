#!/usr/bin/env python
"""Run every form of an adjoint evaluation once (tests/adjoint_forms.py) and print what the library did: per form the launches
per class, the stats() deltas, every contrast and gradient as hex, and one digest over the deterministic forms.  For comparing two
builds of the library (CMAX_HIP_SO selects one per process), plainly or under a tracer:

    python tools/adjoint_forms_walk.py                 # the table tests/test_gpu_adjoint_forms.py asserts
    python tools/adjoint_forms_walk.py --untimed       # the same calls without timing events (what a trace should see)
"""
import argparse
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402

import adjoint_forms as af  # noqa: E402
from cmax_slam_amd import _lib, evaluator  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--untimed", action="store_true")
    ap.add_argument("--only", nargs="*")
    args = ap.parse_args()
    print("library:", _lib.SO_PATH)
    det = hashlib.sha256()
    for kind, name, rec in af.walk(evaluator, timed=not args.untimed, only=args.only):
        tag = "%s %-18s" % ("fe" if kind == "f" else "be", name)
        if "x" in rec:
            print(tag, "x", " ".join("%.6f" % v for v in rec["x"]), "final_cost %.9g" % rec["final_cost"],
                  " ".join("%s=%d" % kv for kv in rec["stats"].items()))
            continue
        print(tag, " ".join("%s=%d" % (k, rec["launches"].get(k, -1)) for k in af.CLASSES), "|",
              " ".join("%s=%d" % (k, rec["stats"][k]) for k in af.STATS))
        for i, c, g in rec["results"]:
            words = [float(c).hex()] + ([float(v).hex() for v in g] if g is not None else [])
            print("    x%d" % i, " ".join(words))
            if name in af.DETERMINISTIC:
                det.update((tag + " ".join(words)).encode())
            c_ref, g_ref = af.expected(kind, name, i)
            err_g = np.abs(g - g_ref).max() / max(np.abs(g_ref).max(), 1e-30) if g is not None else 0.0
            print("       rel. error against the oracle: contrast %.2e gradient %.2e" % (abs(c - c_ref) / max(abs(c_ref), 1e-30), err_g))
    print("digest of the deterministic forms:", det.hexdigest())


if __name__ == "__main__":
    main()
