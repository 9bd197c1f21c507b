#!/usr/bin/env python3
"""Timing of a whole-trajectory binding that grows (cmx_backend_recon_extend / _bind_append_from / _advance_head / _release_head;
DESIGN 4.15) -> profiles/recon_online_timing.txt.

tools/time_recon.py's large configuration -- 20M events over 20 s from the event store, 1280x720 sensor, 4096x2048 panorama, linear
spline with 401 knots, batch 100 -- replayed in strides of --stride-knots knot intervals (2 = 100 ms) with the last --free knots
free.  Per step, host clock around the synchronous calls:
    extend(K)   bind_append_from(the stride's events)   eval_bound with gradient (the first one after an append sorts)
    advance_head(K - free)   release_head()
and, every --parent-every steps and in the same process, what the library offered before for the same step on a second context:
bind_from over everything so far + freeze_head(K - free) (the begin that a longer spline needed there is not counted).  Resident
sampled events after every step, from cmx_backend_recon_online_info.  Needs a GPU."""
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


def timed(fn, *a, **k):
    t0 = time.perf_counter()
    r = fn(*a, **k)
    return time.perf_counter() - t0, r


def med(v):
    return statistics.median(v) if v else float("nan")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--events", type=int, default=20_000_000)
    ap.add_argument("--seconds", type=float, default=20.0)
    ap.add_argument("--sensor", type=int, nargs=2, default=(1280, 720))
    ap.add_argument("--pano", type=int, nargs=2, default=(4096, 2048))
    ap.add_argument("--batch", type=int, default=100)
    ap.add_argument("--sigma", type=float, default=1.0)
    ap.add_argument("--stride-knots", type=int, default=2)
    ap.add_argument("--free", type=int, default=8)
    ap.add_argument("--parent-every", type=int, default=10)
    ap.add_argument("--commit", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "recon_online_timing.txt"))
    a = ap.parse_args()
    from cmax_slam_amd import _lib, evaluator
    assert _lib.lib().cmx_device_count() > 0, "no GPU visible: this tool measures on the device only"
    commit = a.commit
    if not commit:
        try:
            commit = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], stderr=subprocess.DEVNULL).decode().strip()
        except Exception:
            commit = "unknown"
    x, y, t, knots, start_ns, dt_ns, lut = tr.make_inputs(a)
    K_all, order = len(knots), 2
    be = evaluator.BackendEvaluator(a.sensor[0], a.sensor[1], lut, a.pano[0], a.pano[1])
    ref = evaluator.BackendEvaluator(a.sensor[0], a.sensor[1], lut, a.pano[0], a.pano[1])
    store = evaluator.EventStore(a.sensor[0], a.sensor[1], len(x))
    store.push(x, y, t)

    def cut(K):
        return int(np.searchsorted(t, start_ns + (K - order + 1) * dt_ns, side="left"))

    K = a.free + order + a.stride_knots
    n = cut(K)
    be.reconstruct_begin(order, knots[:K], start_ns, dt_ns, a.batch, 1)
    be.reconstruct_bind(store, 0, n)
    be.reconstruct_eval_bound(knots[:K], a.sigma, 0, True)
    be.reconstruct_advance_head(K - a.free)
    be.reconstruct_release_head()
    rows, parent = [], []
    step = 0
    while K < K_all:
        K2 = min(K + a.stride_knots, K_all)
        n2 = cut(K2)
        q = np.ascontiguousarray(knots[:K2])
        r = {"K": K2, "events": n2, "new": n2 - n}
        r["extend"], _ = timed(be.reconstruct_extend, q)
        r["append"], _ = timed(be.reconstruct_bind_append, store, n, n2 - n)
        r["eval_first"], (c1, g1) = timed(be.reconstruct_eval_bound, q, a.sigma, 0, True)
        r["eval"], _ = timed(be.reconstruct_eval_bound, q, a.sigma, 0, True)
        r["advance"], _ = timed(be.reconstruct_advance_head, K2 - a.free)
        r["release"], _ = timed(be.reconstruct_release_head)
        on = be.reconstruct_online_info()
        fi = be.reconstruct_frozen_info()
        r["resident"], r["released"], r["frozen_batches"] = on["resident_sampled"], on["released_sampled"], fi["frozen_batches"]
        r["resident_batches"] = (n2 - 1 + a.batch - 1) // a.batch - on["released_batches"]
        if a.parent_every and (step % a.parent_every == 0 or K2 == K_all):
            ref.reconstruct_begin(order, q, start_ns, dt_ns, a.batch, 1)
            p = {"K": K2, "events": n2}
            p["bind"], _ = timed(ref.reconstruct_bind, store, 0, n2)
            p["freeze"], _ = timed(ref.reconstruct_freeze_head, K2 - a.free)
            p["eval"], (c2, g2) = timed(ref.reconstruct_eval_bound, q, a.sigma, 0, True)
            p["contrast_rel"] = abs(c1 - c2) / abs(c2)
            # (g1 was taken before the advance, under the previous line: the entries free under BOTH heads are compared)
            lo = 3 * (K2 - a.free)
            p["grad_rel"] = float(np.abs(g1[lo:] - g2[lo:]).max() / max(np.abs(g2[lo:]).max(), 1e-300))
            p["same_head"] = ref.reconstruct_frozen_info() == fi
            p["online"] = r["append"] + r["advance"] + r["release"]
            parent.append(p)
            ref.reconstruct_end()
        rows.append(r)
        K, n, step = K2, n2, step + 1
    be.reconstruct_end()
    store.close()

    ms = lambda v: 1e3 * v  # noqa: E731
    L = ["a whole-trajectory binding that grows: cmx_backend_recon_extend / _bind_append_from / _advance_head / _release_head",
         "commit %s; %d events over %.0f s, sensor %dx%d, panorama %dx%d, linear spline of %d knots, batch %d, default mode" %
         (commit, len(x), a.seconds, a.sensor[0], a.sensor[1], a.pano[0], a.pano[1], K_all, a.batch),
         "%d steps of %d knot intervals (%.0f ms of recording, about %d events each), the last %d knots free; host clock around synchronous calls" %
         (len(rows), a.stride_knots, 1e-6 * a.stride_knots * dt_ns, int(med([r["new"] for r in rows])), a.free), "",
         "per step, ms (median / first / last / max over the steps)"]
    for k in ("extend", "append", "eval_first", "eval", "advance", "release"):
        v = [ms(r[k]) for r in rows]
        L.append("  %-12s %8.3f %8.3f %8.3f %8.3f" % (k, med(v), v[0], v[-1], max(v)))
    v = [ms(r["append"] + r["advance"] + r["release"]) for r in rows]
    L.append("  %-12s %8.3f %8.3f %8.3f %8.3f   (append + advance + release: the book-keeping of a step)" %
             ("step", med(v), v[0], v[-1], max(v)))
    half = len(rows) // 2
    L += ["  the book-keeping over the first half of the run %.3f ms, over the second half %.3f ms (median): events bound so far %d -> %d" %
          (med(v[:half]), med(v[half:]), rows[0]["events"], rows[-1]["events"]), ""]
    res = [r["resident"] for r in rows]
    byt = [16 * r["resident"] + 80 * r["resident_batches"] for r in rows]
    L += ["resident sampled events after release: min %d, median %d, max %d (of %d bound at the end, %d released)" %
          (min(res), int(med(res)), max(res), rows[-1]["events"] - 1, rows[-1]["released"]),
          "  at 16 bytes per sampled event and 80 per batch: %.2f MB at most (live entries; the arrays hold up to twice that between moves); the whole recording bound would hold %.1f MB" %
          (1e-6 * max(byt), 1e-6 * (16 * (rows[-1]["resident"] + rows[-1]["released"]) + 80 * ((rows[-1]["events"] + a.batch - 1) // a.batch))),
          "", "the same step the way it was done before: bind_from over everything so far + freeze_head, same process, every %d steps" % a.parent_every,
          "%8s %12s %10s %10s %12s %12s %10s %10s" % ("K", "events", "bind ms", "freeze ms", "bind+freeze", "online step", "ratio", "same head")]
    for p in parent:
        L.append("%8d %12d %10.3f %10.3f %12.3f %12.3f %10.1f %10s" %
                 (p["K"], p["events"], ms(p["bind"]), ms(p["freeze"]), ms(p["bind"] + p["freeze"]), ms(p["online"]),
                  (p["bind"] + p["freeze"]) / p["online"], p["same_head"]))
    L += ["  evaluation under the grown binding against the fresh one at the same knots: contrast rel %.2e, gradient rel %.2e (max over the rows; "
          "default mode: equal to summation order)" % (max(p["contrast_rel"] for p in parent), max(p["grad_rel"] for p in parent)),
          "  first eval_bound with gradient (it sorts), fresh binding with the same head: %.3f ms (median); grown binding: %.3f ms" %
          (med([ms(p["eval"]) for p in parent[1:]]), med([ms(r["eval_first"]) for r in rows])), ""]
    text = "\n".join(L)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
