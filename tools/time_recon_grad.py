#!/usr/bin/env python3
"""Whole-trajectory contrast and gradient (cmx_backend_recon_restart / _contrast / _grad_add_from / _grad_get / _eval_from), phase by
phase, and the same evaluation over events bound once (cmx_backend_recon_bind_from / _eval_bound), in one run on one GPU.

  (large)   tools/time_recon.py's configuration: 20M events from the event store, 1280x720 sensor, 4096x2048 panorama, linear spline
            with 401 knots, batch 100.  Median of --reps runs per phase after --warmup warm-up runs, host clock around synchronous
            calls: restart, add_from (the vote pass: the kernel profiles/recon_timing.txt records), contrast cost-only, contrast with
            gradient, grad_add_from (the gather pass), grad_get, and the whole eval_from with and without the gradient.  Then, in the
            same process on the same events: bind_from, the first eval_bound (the one that sorts), steady-state eval_bound cost-only
            and with the gradient, eval_bound at knots moved by N(0, 1 mrad) with the share of votes that left their windows, the
            pose-table, tile-sort and vote kernels by their own events (cmx_timing_enable), and the break-even number of
            evaluations (bind + sort) / (eval_from - eval_bound).
  (window)  config 3 (5M events, cubic K = 10, 1024 x 1024): reconstruct_eval with the gradient against the window path's
            set_window_from + one eval with the gradient (num_fixed = 0, no map), and against eval_bound on the same events.
  (pmc)     the large configuration once under rocprofv3 --pmc, one counter group per run: VALU instructions of the gather and
            vote kernels per event, and the atomic requests that reach the L2.
  (solve)   the large configuration again, all rows in one process (--only-solve: this step alone): reconstruct_refine(bind=True)
            against reconstruct_solve from the same start, whole and per evaluation, in default and in deterministic mode, with
            the host waits per evaluation the library counted; eval_bound with the gradient under frozen heads of num_fixed = 0,
            K/2, 3K/4 and K - 8 with the vote and gather passes by their own events, the one-off cost of the freeze and its
            break-even.  Written to profiles/recon_solve_timing.txt (--solve-out).

No threshold is fixed: the file states the ratios.  Every step runs in a child process of its own, in a process group of its own,
under a time limit; a child that ends with a non-zero status or at its limit is the LAST thing this tool starts on the GPU.
Writes profiles/recon_bound_timing.txt (--out).  Needs a GPU; there is no fallback."""
import argparse
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402

import time_recon as tr  # noqa: E402  (the stream of the large configuration, the child runner, the CSV reader)


def med(v):
    return statistics.median(v) if v else float("nan")


def timed(fn, *a, **k):
    t0 = time.perf_counter()
    r = fn(*a, **k)
    return time.perf_counter() - t0, r


def step_large(a):
    from cmax_slam_amd import evaluator
    x, y, t, knots, start_ns, dt_ns, lut = tr.make_inputs(a)
    be = evaluator.BackendEvaluator(a.sensor[0], a.sensor[1], lut, a.pano[0], a.pano[1])
    store = evaluator.EventStore(a.sensor[0], a.sensor[1], len(x))
    store.push(x, y, t)
    n = len(x)
    ph = {k: [] for k in ("restart", "add_from", "contrast_cost", "contrast_grad", "grad_add_from", "grad_get", "eval_cost", "eval_grad")}
    be.reconstruct_begin(2, knots, start_ns, dt_ns, a.batch, 1)
    c = g = None
    for i in range(a.warmup + a.reps):
        s = {}
        s["restart"], _ = timed(be.reconstruct_restart, knots)
        s["add_from"], _ = timed(be.reconstruct_add_from, store, 0, n)
        s["contrast_cost"], _ = timed(be.reconstruct_contrast, a.sigma, 0, False)
        s["contrast_grad"], c = timed(be.reconstruct_contrast, a.sigma, 0, True)
        s["grad_add_from"], _ = timed(be.reconstruct_grad_add_from, store, 0, n)
        s["grad_get"], g = timed(be.reconstruct_grad_get)
        s["eval_cost"], _ = timed(be.reconstruct_eval, store, 0, n, knots, a.sigma, 0, False)
        s["eval_grad"], (c2, g2) = timed(be.reconstruct_eval, store, 0, n, knots, a.sigma, 0, True)
        if i >= a.warmup:
            for k, v in s.items():
                ph[k].append(v)
    _, ns, ni = be.reconstruct_get(with_counts=True)
    # ---- the same events bound once, evaluated through the tile sort and LDS votes
    from scipy.spatial.transform import Rotation as Rot
    moved = (Rot.from_rotvec(np.random.default_rng(5).normal(0, 1e-3, (len(knots), 3))) * Rot.from_quat(knots)).as_quat()
    bp = {k: [] for k in ("bind", "first_eval", "bound_cost", "bound_grad", "bound_moved")}
    frac_moved = 0.0
    rounds = a.warmup + a.reps
    for i in range(rounds):
        s = {}
        s["bind"], _ = timed(be.reconstruct_bind, store, 0, n)
        s["first_eval"], _ = timed(be.reconstruct_eval_bound, knots, a.sigma, 0, True)
        s["bound_cost"], _ = timed(be.reconstruct_eval_bound, knots, a.sigma, 0, False)
        s["bound_grad"], (cb, gb) = timed(be.reconstruct_eval_bound, knots, a.sigma, 0, True)
        s["bound_moved"], _ = timed(be.reconstruct_eval_bound, moved, a.sigma, 0, True)
        frac_moved = be.reconstruct_bound_info()["fallback_frac"]
        if i >= a.warmup:
            for k, v in s.items():
                bp[k].append(v)
    extra = max(a.reps, 1)
    be.timing_enable(["pose", "batch", "splat"])  # the bound path's kernels by their own events, in evaluations of their own
    be.reconstruct_bind(store, 0, n)
    for i in range(extra):
        be.reconstruct_eval_bound(knots, a.sigma, 0, True)
    tm = be.timing_get()
    be.timing_enable(False)
    info = be.reconstruct_bound_info()
    _, nsb, nib = be.reconstruct_get(with_counts=True)
    be.reconstruct_end()
    bound = {"phases": {k: med(v) for k, v in bp.items()}, "contrast_rel": abs(cb - c2) / abs(c2),
             "grad_rel": float(np.abs(gb - g2).max() / np.abs(g2).max()), "sampled": nsb, "inside": nib, "sorts": info["sorts"],
             "fallback_frac": info["fallback_frac"], "fallback_frac_moved": frac_moved,
             "kernels": {k: [tm[k][0], tm[k][1]] for k in ("pose", "batch", "splat")},
             # passes over the sampled events this process made, per kernel (the per-event figures of a profiled run)
             "passes": {"recon_votes_kernel": 3 * rounds, "recon_votes_lds": 4 * rounds + extra, "recon_gather": 5 * rounds + extra}}
    out = {"events": n, "K": len(knots), "sampled": ns, "inside": ni, "contrast": c, "gmax": float(np.abs(g).max()),
           "eval_vs_phases": float(np.abs(g2 - g).max()), "phases": {k: med(v) for k, v in ph.items()}, "bound": bound}
    print("RESULT " + json.dumps(out), flush=True)


def step_window(a):
    from cmax_slam_amd import evaluator, synth
    w = synth.config3()
    be = evaluator.BackendEvaluator(w.W, w.H, w.lut, w.Wp, w.Hp)
    n = len(w.x)
    store = evaluator.EventStore(w.W, w.H, n)
    store.push(w.x, w.y, w.t_ns)
    t_all = int(w.t_ns[-1]) + 1
    win_set, win_eval, rec = [], [], []
    zero = np.zeros(3 * len(w.knots_init))
    be.reconstruct_begin(w.order, w.knots_init, w.start_ns, w.dt_ns, 100, 1)
    for i in range(a.warmup + a.reps):
        t0, _ = timed(be.set_window_from, store, 0, n, w.order, w.knots_init, w.start_ns, w.dt_ns, 0, t_all, 100, 1, blur_sigma=a.sigma)
        t1, (cw, gw) = timed(be.eval, zero, True)
        t2, (cr, gr) = timed(be.reconstruct_eval, store, 0, n, w.knots_init, a.sigma, 0, True)
        if i >= a.warmup:
            win_set.append(t0); win_eval.append(t1); rec.append(t2)
    bnd = []
    t_bind, _ = timed(be.reconstruct_bind, store, 0, n)
    t_first, _ = timed(be.reconstruct_eval_bound, w.knots_init, a.sigma, 0, True)
    for i in range(a.warmup + a.reps):
        t3, (cb, gb) = timed(be.reconstruct_eval_bound, w.knots_init, a.sigma, 0, True)
        if i >= a.warmup:
            bnd.append(t3)
    be.reconstruct_end()
    out = {"events": n, "set_window_from": med(win_set), "eval": med(win_eval), "reconstruct_eval": med(rec),
           "bind": t_bind, "first_eval_bound": t_first, "eval_bound": med(bnd),
           "bound_grad_rel": float(np.abs(np.array(gb) - gw).max() / np.abs(gw).max()),
           "contrast_rel": abs(cr - cw) / abs(cw), "grad_rel": float(np.abs(np.array(gr) - gw).max() / np.abs(gw).max())}
    print("RESULT " + json.dumps(out), flush=True)


def step_solve(a):
    """The bundle adjustment over the large configuration, all rows in this one process: (a) reconstruct_refine(bind=True), the Python
    loop around cmx_frcg_minimize; (b) reconstruct_solve(freeze_head=False), the native call, from the same start; (c) eval_bound with
    the gradient under frozen heads of several lengths, with the vote and gather passes by their own events and the one-off cost of
    the freeze; (d) the host waits per evaluation of (b), as the library counted them."""
    from cmax_slam_amd import evaluator
    x, y, t, knots, start_ns, dt_ns, lut = tr.make_inputs(a)
    n, K = len(x), len(knots)
    from scipy.spatial.transform import Rotation as Rot
    start = np.ascontiguousarray((Rot.from_rotvec(np.random.default_rng(5).normal(0, 1e-3, (K, 3))) * Rot.from_quat(knots)).as_quat())
    store = evaluator.EventStore(a.sensor[0], a.sensor[1], n)
    store.push(x, y, t)
    out = {"events": n, "K": K, "modes": {}}
    for det in (False, True):
        be = evaluator.BackendEvaluator(a.sensor[0], a.sensor[1], lut, a.pano[0], a.pano[1])
        if det:
            be.set_deterministic(True)
        py, nat, nat_call, waits = [], [], [], None
        rp = rn = kp = kn = None
        for i in range(a.warmup + a.reps):  # alternating: a Python-route solve, then a native one
            dt_py, (kp, rp) = timed(be.reconstruct_refine, store, 0, n, 2, start, start_ns, dt_ns, 1, a.sigma, 0, a.batch, 1, True)
            t0 = time.perf_counter()
            be.reconstruct_begin(2, start, start_ns, dt_ns, a.batch, 1)
            be.reconstruct_bind(store, 0, n)
            dt_call, (kn, rn) = timed(be.reconstruct_solve, start, 1, a.sigma, 0, False)
            waits = be.reconstruct_solve_counts()
            be.reconstruct_end()
            dt_nat = time.perf_counter() - t0
            if i >= a.warmup:
                py.append(dt_py); nat.append(dt_nat); nat_call.append(dt_call)
        out["modes"]["deterministic" if det else "default"] = {
            "python_s": med(py), "native_s": med(nat), "native_call_s": med(nat_call), "python_report": rp, "native_report": rn,
            "same_knots": bool(kp.tobytes() == kn.tobytes()), "max_dq": float(np.abs(kp - kn).max()), "evals_waits": list(waits)}
        be.close()
    # ---- (c) frozen heads, default mode
    be = evaluator.BackendEvaluator(a.sensor[0], a.sensor[1], lut, a.pano[0], a.pano[1])
    be.reconstruct_begin(2, knots, start_ns, dt_ns, a.batch, 1)
    be.reconstruct_bind(store, 0, n)
    rows = []
    g0 = None
    for nf in (0, K // 2, 3 * K // 4, K - 8):
        fr = []
        for i in range(3):  # (the freeze is paid once per solve: three calls, their median)
            be.reconstruct_freeze_head(0)
            be.reconstruct_restart(knots)
            dt_f, _ = timed(be.reconstruct_freeze_head, nf)
            fr.append(dt_f)
        info = be.reconstruct_frozen_info()
        cost, grad = [], []
        for i in range(a.warmup + a.reps):
            t_c, _ = timed(be.reconstruct_eval_bound, knots, a.sigma, 0, False)
            t_g, (c, g) = timed(be.reconstruct_eval_bound, knots, a.sigma, 0, True)
            if i >= a.warmup:
                cost.append(t_c); grad.append(t_g)
        if nf == 0:
            g0 = g
        be.timing_enable(["pose", "batch", "splat", "gather"])
        for i in range(max(a.reps, 1)):
            be.reconstruct_eval_bound(knots, a.sigma, 0, True)
        tm = be.timing_get()
        be.timing_enable(False)
        rows.append({"num_fixed": nf, "freeze_s": med(fr), "frozen_batches": info["frozen_batches"], "frozen_sampled": info["frozen_sampled"],
                     "cost_s": med(cost), "grad_s": med(grad), "evals": max(a.reps, 1),
                     "kernels": {k: [tm[k][0], tm[k][1]] for k in ("pose", "batch", "splat", "gather")},
                     "grad_rel": float(np.abs(g[3 * nf:] - g0[3 * nf:]).max() / np.abs(g0).max()), "fixed_zero": bool(not g[:3 * nf].any())})
    out["sampled"] = be.reconstruct_bound_info()["n_sampled"]
    be.reconstruct_end()
    out["frozen"] = rows
    print("RESULT " + json.dumps(out), flush=True)


def write_solve(a, commit, sv):
    n, K = sv["events"], sv["K"]
    L = ["whole-trajectory bundle adjustment as one native call, and the frozen head: cmx_backend_recon_solve / _freeze_head",
         "commit: %s    %d events from the event store, %dx%d sensor, %dx%d panorama, linear spline with %d knots, batch %d, rate 1, sigma %g" %
         (commit, n, a.sensor[0], a.sensor[1], a.pano[0], a.pano[1], K, a.batch, a.sigma),
         "median of %d runs after %d warm-up runs, all rows in one process; host clock around synchronous calls" % (a.reps, a.warmup),
         "start: the stream's knots moved by N(0, 1 mrad) per component, num_fixed = 1, the back end's solver constants", ""]
    for mode, m in sv["modes"].items():
        rp, rn = m["python_report"], m["native_report"]
        ep, en = rp["n_f"] + rp["n_df"], rn["n_f"] + rn["n_df"]
        L += ["%s mode:" % mode,
              "  (a) reconstruct_refine(bind=True): begin + bind + solve + end %10.3f ms; %d iterations, %d evaluations: %.3f ms per evaluation" %
              (1e3 * m["python_s"], rp["iterations"], ep, 1e3 * m["python_s"] / max(ep, 1)),
              "  (b) begin + bind + reconstruct_solve(freeze_head=False) + end %10.3f ms; %d iterations, %d evaluations: %.3f ms per evaluation"
              % (1e3 * m["native_s"], rn["iterations"], en, 1e3 * m["native_s"] / max(en, 1)),
              "      of which the solve call alone %.3f ms: %.3f ms per evaluation" % (1e3 * m["native_call_s"], 1e3 * m["native_call_s"] / max(en, 1)),
              "      (b) / (a), whole: %.3f; per evaluation: %.3f; same knots byte for byte: %s (max |dq| %.2e)" %
              (m["native_s"] / m["python_s"], (m["native_s"] / max(en, 1)) / (m["python_s"] / max(ep, 1)), m["same_knots"], m["max_dq"]),
              "  (d) host waits inside the evaluations of (b), counted by the library: %d waits in %d evaluations = %.3f per evaluation" %
              (m["evals_waits"][1], m["evals_waits"][0], m["evals_waits"][1] / max(m["evals_waits"][0], 1)), ""]
    L += ["(c) eval_bound under a frozen head, default mode, at the knots of the freeze; kernels by their own events over %d evaluations of "
          "their own (vote: the dispatch's timestamps; gather: events on the stream around each slice's launches); %d sampled events" %
          (sv["frozen"][0]["evals"], sv["sampled"]),
          "%-10s %10s %12s %10s %10s %10s %10s %10s %10s" % ("num_fixed", "batches", "active share", "freeze ms", "cost ms", "grad ms", "vote ms",
                                                           "gather ms", "pose ms")]
    base = sv["frozen"][0]

    def per(r, k):
        return r["kernels"][k][0] / r["evals"]
    for r in sv["frozen"]:
        L.append("%-10d %10d %12.4f %10.3f %10.3f %10.3f %10.3f %10.3f %10.3f" %
                 (r["num_fixed"], r["frozen_batches"], 1.0 - r["frozen_sampled"] / sv["sampled"], 1e3 * r["freeze_s"], 1e3 * r["cost_s"],
                  1e3 * r["grad_s"], per(r, "splat"), per(r, "gather"), per(r, "pose")))
    L.append("")
    for r in sv["frozen"][1:]:
        gain = base["grad_s"] - r["grad_s"]
        L.append("num_fixed %d against num_fixed 0 of this run: vote %.3f x, gather %.3f x, eval_bound with gradient %.3f x, cost only %.3f x; "
                 "break-even of the freeze: %s; free gradient against the unfrozen one %.2e (max-norm), fixed entries zero: %s" %
                 (r["num_fixed"], per(r, "splat") / per(base, "splat"), per(r, "gather") / per(base, "gather"), r["grad_s"] / base["grad_s"],
                  r["cost_s"] / base["cost_s"], "%.1f evaluations with gradient" % (r["freeze_s"] / gain) if gain > 0 else
                  "never: the frozen evaluation is not faster", r["grad_rel"], r["fixed_zero"]))
    text = "\n".join(L) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.solve_out)), exist_ok=True)
    with open(a.solve_out, "w") as f:
        f.write(text)
    print(text)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", default=None, choices=(None, "large", "window", "solve"))
    ap.add_argument("--only-solve", action="store_true", help="the solve / frozen-head rows alone (profiles/recon_solve_timing.txt)")
    ap.add_argument("--solve-out", default=os.path.join(ROOT, "profiles", "recon_solve_timing.txt"))
    ap.add_argument("--events", type=int, default=20_000_000)
    ap.add_argument("--seconds", type=float, default=20.0)
    ap.add_argument("--sensor", type=int, nargs=2, default=(1280, 720))
    ap.add_argument("--pano", type=int, nargs=2, default=(4096, 2048))
    ap.add_argument("--batch", type=int, default=100)
    ap.add_argument("--sigma", type=float, default=1.0)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-profile", action="store_true", help="skip the rocprofv3 counter runs")
    ap.add_argument("--commit", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "recon_bound_timing.txt"))
    a = ap.parse_args()
    if a.step == "large":
        return step_large(a)
    if a.step == "window":
        return step_window(a)
    if a.step == "solve":
        return step_solve(a)

    from cmax_slam_amd import _lib
    assert _lib.lib().cmx_device_count() > 0, "no GPU visible: this tool measures on the device only"
    commit = a.commit
    if not commit:
        try:
            commit = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], stderr=subprocess.DEVNULL).decode().strip()
        except Exception:
            commit = "unknown"

    def child(step, extra=(), wrap=(), limit=420):
        # (time_recon's runner starts its own file: point it at this one)
        saved = tr.__file__
        tr.__file__ = os.path.abspath(__file__)
        try:
            return tr.child(a, step, ["--sigma", str(a.sigma)] + list(extra), wrap, limit)
        finally:
            tr.__file__ = saved

    if a.only_solve:
        write_solve(a, commit, child("solve", limit=900))
        return 0
    big = child("large")  # (a timing child that dies ends the run: ChildDied propagates, nothing further is started)
    win = child("window")
    write_solve(a, commit, child("solve", limit=900))
    n, p = big["events"], big["phases"]
    L = ["whole-trajectory contrast and gradient: cmx_backend_recon_restart / _contrast / _grad_add_from / _grad_get / _eval_from, and "
         "the same over bound events: _bind_from / _eval_bound",
         "commit: %s    %d events from the event store, %dx%d sensor, %dx%d panorama, linear spline with %d knots, batch %d, rate 1, sigma %g" %
         (commit, n, a.sensor[0], a.sensor[1], a.pano[0], a.pano[1], big["K"], a.batch, a.sigma),
         "median of %d runs after %d warm-up runs; host clock around synchronous calls" % (a.reps, a.warmup),
         "sampled %d, voted %d; contrast %.6g, |grad|max %.4g; eval_from against the phase-by-phase gradient: max |diff| %.2e" %
         (big["sampled"], big["inside"], big["contrast"], big["gmax"], big["eval_vs_phases"]),
         "",
         "%-58s %10s %14s" % ("phase", "ms", "events/s")]
    for k, label in (("restart", "restart (knots, zero the plane)"), ("add_from", "add_from (vote pass)"),
                     ("contrast_cost", "contrast, cost only (tile flags, list, moments)"),
                     ("contrast_grad", "contrast with gradient (tile flags, list, adjoint pass)"),
                     ("grad_add_from", "grad_add_from (gather pass)"), ("grad_get", "grad_get (2 x 3K sums to the host)"),
                     ("eval_cost", "eval_from, cost only"), ("eval_grad", "eval_from, with gradient")):
        L.append("%-58s %10.3f %14.3e" % (label, 1e3 * p[k], n / p[k]))
    bd = big["bound"]
    q, kt = bd["phases"], bd["kernels"]
    for k, label in (("bind", "bind_from (batch times, packed copy, the sort's buffers)"),
                     ("first_eval", "eval_bound with gradient, the first (tile sort included)"),
                     ("bound_cost", "eval_bound, cost only, steady state"), ("bound_grad", "eval_bound, with gradient, steady state"),
                     ("bound_moved", "eval_bound, with gradient, knots moved by N(0, 1 mrad)")):
        L.append("%-58s %10.3f %14.3e" % (label, 1e3 * q[k], n / q[k]))

    def each(v):
        return v[0] / v[1] if v[1] else float("nan")
    sort_ms = 1e3 * (q["first_eval"] - q["bound_grad"])
    gain_ms = 1e3 * (p["eval_grad"] - q["bound_grad"])
    L += ["",
          "bound path, kernels by their own events (%d evaluations of their own): pose table %.3f ms, tile sort + chunk table %.3f ms "
          "(%d run), vote kernel %.3f ms" % (kt["splat"][1], each(kt["pose"]), each(kt["batch"]), kt["batch"][1], each(kt["splat"])),
          "bound path: sampled %d, voted %d, tile sorts since the last bind %d; votes outside their window: %.4f at the sort's knots, "
          "%.4f with the knots moved by 1 mrad" % (bd["sampled"], bd["inside"], bd["sorts"], bd["fallback_frac"], bd["fallback_frac_moved"]),
          "eval_bound against eval_from at the same knots: contrast %.2e, gradient %.2e (relative, max-norm)" %
          (bd["contrast_rel"], bd["grad_rel"]),
          "eval_from with gradient / eval_bound with gradient, steady state: %.2f x" % (p["eval_grad"] / q["bound_grad"]),
          "break-even: (bind %.3f ms + sort %.3f ms) / (eval_from %.3f ms - eval_bound %.3f ms) = %s" %
          (1e3 * q["bind"], sort_ms, 1e3 * p["eval_grad"], 1e3 * q["bound_grad"],
           "%.1f evaluations" % ((1e3 * q["bind"] + sort_ms) / gain_ms) if gain_ms > 0 else "never: eval_bound is not faster"),
          "",
          "gather pass / vote pass of the same run: %.2f x" % (p["grad_add_from"] / p["add_from"]),
          "eval_from with gradient / cost only: %.2f x" % (p["eval_grad"] / p["eval_cost"]),
          "",
          "config 3 (%d events, cubic K = 10, 1024 x 1024), num_fixed = 0, no map:" % win["events"],
          "  window path: set_window_from %.3f ms + eval with gradient %.3f ms = %.3f ms" %
          (1e3 * win["set_window_from"], 1e3 * win["eval"], 1e3 * (win["set_window_from"] + win["eval"])),
          "  reconstruct_eval with gradient (restart + add_from + contrast + grad_add_from + grad_get): %.3f ms" % (1e3 * win["reconstruct_eval"]),
          "  reconstruct_eval / (set_window_from + eval): %.2f x;  / eval alone: %.2f x" %
          (win["reconstruct_eval"] / (win["set_window_from"] + win["eval"]), win["reconstruct_eval"] / win["eval"]),
          "  agreement of the two: contrast %.2e, gradient %.2e (relative, max-norm)" % (win["contrast_rel"], win["grad_rel"]),
          "  bound: bind_from %.3f ms, first eval_bound (sort included) %.3f ms, eval_bound with gradient, steady state %.3f ms" %
          (1e3 * win["bind"], 1e3 * win["first_eval_bound"], 1e3 * win["eval_bound"]),
          "  eval_bound / (set_window_from + eval): %.2f x;  / eval alone: %.2f x;  its gradient against the window path's: %.2e" %
          (win["eval_bound"] / (win["set_window_from"] + win["eval"]), win["eval_bound"] / win["eval"], win["bound_grad_rel"])]
    died = None
    if not a.no_profile and not shutil.which("rocprofv3"):
        L += ["", "rocprofv3 is not installed: no counters"]
    elif not a.no_profile:
        one = ["--reps", "1", "--warmup", "0"]
        for grp in ("SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_LDS SQ_WAVES", "TCC_ATOMIC_sum TCC_READ_sum TCC_WRITE_sum"):
            if died:
                break
            with tempfile.TemporaryDirectory(prefix="recon_grad_pmc_") as d:
                try:
                    prof = child("large", one, ["rocprofv3", "--pmc"] + grp.split() + ["--output-format", "csv", "-d", d, "-o", "rg", "--"],
                                 limit=300)
                    passes = prof["bound"]["passes"]  # (of the profiled run itself)
                    for kern in ("recon_gather", "recon_votes_kernel", "recon_votes_lds"):
                        acc = {}
                        for r in tr.rows_of(d, "counter_collection.csv"):
                            if kern in r.get("Kernel_Name", "") and "rows" not in r.get("Kernel_Name", ""):
                                acc[r["Counter_Name"]] = acc.get(r["Counter_Name"], 0.0) + float(r["Counter_Value"])
                        L.append("PMC (a run of its own), %s launches summed: " % kern + ", ".join("%s %.4g" % kv for kv in sorted(acc.items())))
                        per = float(passes[kern]) * big["sampled"]  # (every pass of the profiled run is over the sampled events)
                        if acc.get("SQ_INSTS_VALU"):
                            L.append("    %s: %.1f VALU instructions per event (wave instructions x 64 lanes / events)" %
                                     (kern, 64.0 * acc["SQ_INSTS_VALU"] / per))
                        if acc.get("TCC_ATOMIC_sum") is not None and "TCC_ATOMIC_sum" in acc:
                            L.append("    %s: %.4g atomic requests at the L2 = %.4f per event" % (kern, acc["TCC_ATOMIC_sum"], acc["TCC_ATOMIC_sum"] / per))
                except tr.ChildDied as e:
                    died = str(e).splitlines()[0]
                except Exception as e:
                    L.append("PMC %s: not readable (%s)" % (grp, str(e).splitlines()[0]))
        if died:
            L += ["", "PROFILING STOPPED, nothing further was started on the GPU: " + died]
    text = "\n".join(L) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(text)
    return 1 if died else 0


if __name__ == "__main__":
    sys.exit(main())
