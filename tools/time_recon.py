#!/usr/bin/env python3
"""Whole-trajectory reconstruction: the new entry points against the route the window ABI offers, in one run on one GPU.

  (new)    cmx_backend_recon_begin / _add (host arrays) or _add_from (event store) / _get: one plane, spline of any length
  (window) what a host had to do before: cut the recording into windows of at most 61 segments, cmx_backend_set_window with
           sigma = 0 and every knot fixed, a cost-only cmx_backend_eval, two cmx_backend_get_plane fetches, a host add

Default size: 20M events, 1280x720 sensor, 4096x2048 panorama, linear spline with 401 knots (20 s at 0.05 s), batch 100.  The
stream is synthetic (uniform sensor pixels, a 360-degree pan with a wobble): only its size and spread matter here.  The window
route is timed twice, from host arrays (cmx_backend_set_window) and from the event store (cmx_backend_set_window_from), so that
each new route has its like-for-like partner.  A step reports the median of --reps runs after --warmup warm-up runs, host clock
around synchronous calls.  A further child runs the new path once under `rocprofv3 --kernel-trace --stats`, and a few more
collect hardware counters, one counter group per run.

Every step runs in a child process of its own, in a process group of its own, under a time limit; at the limit the whole group
is killed.  A child that ends with a non-zero status or at its limit (ChildDied) is the LAST thing this tool starts on the GPU:
a timing child that dies ends the run, a profiling child that dies ends the profiling -- what was measured until then is
written, with a note, and the exit status is 1.  A profiler that is not installed, or output that cannot be parsed after a
clean exit, only costs that section.
Writes profiles/recon_timing.txt (--out).  Needs a GPU; there is no fallback."""
import argparse
import csv
import glob
import json
import os
import shutil
import signal
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

DT = 0.05
SEG = 61             # segments per window of the old route (62 knots of a linear spline; the window ABI takes at most 64)
ATOMIC_PEAK = 1.3e12  # bytes/s of fp32 atomic adds the MI355X retires chip-wide (memory-side execution)
HBM_PEAK = 8.0e12     # bytes/s


def make_inputs(a):
    from scipy.spatial.transform import Rotation as Rot
    from cmax_slam_amd import synth
    rng = np.random.default_rng(11)
    n, W, H = a.events, a.sensor[0], a.sensor[1]
    K = int(round(a.seconds / DT)) + 1
    ang = 2 * np.pi * np.arange(K) / (K - 1)
    knots = (Rot.from_rotvec(np.c_[0.1 * np.sin(3 * ang), ang, 0.05 * np.cos(2 * ang)])).as_quat()
    start_ns, dt_ns = 1_000_000_000, int(DT * 1e9)
    t = start_ns + np.sort(rng.integers(0, (K - 1) * dt_ns, n, dtype=np.int64))
    x = rng.integers(0, W, n, dtype=np.uint16)
    y = rng.integers(0, H, n, dtype=np.uint16)
    f = 0.9 * W
    lut = synth.pinhole_lut(W, H, f, f, (W - 1) / 2, (H - 1) / 2)
    return x, y, t, knots, start_ns, dt_ns, lut


def med(v):
    return statistics.median(v) if v else float("nan")


def step_new(a):
    from cmax_slam_amd import evaluator
    x, y, t, knots, start_ns, dt_ns, lut = make_inputs(a)
    be = evaluator.BackendEvaluator(a.sensor[0], a.sensor[1], lut, a.pano[0], a.pano[1])
    store = evaluator.EventStore(a.sensor[0], a.sensor[1], len(x))
    store.push(x, y, t)
    out = {"events": len(x), "K": len(knots)}
    for how in ("host", "store"):
        whole, add = [], []
        for i in range(a.warmup + a.reps):
            t0 = time.perf_counter()
            be.reconstruct_begin(2, knots, start_ns, dt_ns, a.batch, 1)
            t1 = time.perf_counter()
            if how == "host":
                be.reconstruct_add(x, y, t)
            else:
                be.reconstruct_add_from(store, 0, len(x))
            t2 = time.perf_counter()
            plane, ns, ni = be.reconstruct_get(with_counts=True)
            t3 = time.perf_counter()
            be.reconstruct_end()
            if i >= a.warmup:
                whole.append(t3 - t0)
                add.append(t2 - t1)
        out[how] = {"whole_s": med(whole), "add_s": med(add), "sampled": ns, "inside": ni, "votes": float(plane.sum(dtype=np.float64))}
    print("RESULT " + json.dumps(out), flush=True)


def step_window(a):
    from cmax_slam_amd import _lib, evaluator
    x, y, t, knots, start_ns, dt_ns, lut = make_inputs(a)
    be = evaluator.BackendEvaluator(a.sensor[0], a.sensor[1], lut, a.pano[0], a.pano[1])
    store = evaluator.EventStore(a.sensor[0], a.sensor[1], len(x))
    store.push(x, y, t)
    K = len(knots)
    wins = []
    for s in range(0, K - 1, SEG):
        e = min(s + SEG, K - 1)
        lo, hi = np.searchsorted(t, [start_ns + s * dt_ns, start_ns + e * dt_ns])
        wins.append((s, e, int(lo), int(hi)))
    out = {"windows": len(wins)}
    for how in ("host", "store"):
        runs = []
        for i in range(a.warmup + a.reps):
            t0 = time.perf_counter()
            total = np.zeros((a.pano[1], a.pano[0]), np.float32)
            for s, e, lo, hi in wins:
                k = knots[s:e + 1]
                if how == "host":
                    be.set_window(x[lo:hi], y[lo:hi], t[lo:hi], 2, k, start_ns + s * dt_ns, dt_ns, len(k), 2 ** 62, a.batch, 1, blur_sigma=0.0)
                else:
                    be.set_window_from(store, lo, hi - lo, 2, k, start_ns + s * dt_ns, dt_ns, len(k), 2 ** 62, a.batch, 1, blur_sigma=0.0)
                be.eval(np.zeros(0), want_grad=False)
                total += be.get_plane(_lib.PLANE_IL_OLD)
                total += be.get_plane(_lib.PLANE_IL_NEW)
            if i >= a.warmup:
                runs.append(time.perf_counter() - t0)
        out[how] = {"whole_s": med(runs), "votes": float(total.sum(dtype=np.float64))}
    print("RESULT " + json.dumps(out), flush=True)


class ChildDied(RuntimeError):
    """A child ended with a non-zero status or was killed at its time limit: nothing more is started on the GPU."""


def child(a, step, extra=(), wrap=(), limit=420):
    cmd = list(wrap) + [sys.executable, os.path.abspath(__file__), "--step", step, "--events", str(a.events), "--seconds", str(a.seconds),
                        "--sensor", str(a.sensor[0]), str(a.sensor[1]), "--pano", str(a.pano[0]), str(a.pano[1]), "--batch", str(a.batch),
                        "--reps", str(a.reps), "--warmup", str(a.warmup)] + list(extra)
    # a session (hence a process group) of its own: under a profiler the process that holds the GPU is a grandchild, and the
    # limit has to end it too
    p = subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, cwd=ROOT, start_new_session=True)
    try:
        raw, _ = p.communicate(timeout=limit)
    except subprocess.TimeoutExpired:
        try:
            os.killpg(p.pid, signal.SIGKILL)
        except ProcessLookupError:
            pass
        p.communicate()
        raise ChildDied("step %s was killed at its limit of %d s" % (step, limit))
    text = raw.decode(errors="replace")
    if p.returncode != 0:
        raise ChildDied("step %s ended with status %d:\n%s" % (step, p.returncode, text[-2000:]))
    for line in text.splitlines():
        if line.startswith("RESULT "):
            return json.loads(line[7:])
    raise RuntimeError("step %s printed no result:\n%s" % (step, text[-2000:]))


def rows_of(d, suffix):
    rows = []
    for p in glob.glob(os.path.join(d, "**", "*" + suffix), recursive=True):
        with open(p, newline="") as f:
            rows += list(csv.DictReader(f))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", default=None, choices=(None, "new", "window"))
    ap.add_argument("--events", type=int, default=20_000_000)
    ap.add_argument("--seconds", type=float, default=20.0)
    ap.add_argument("--sensor", type=int, nargs=2, default=(1280, 720))
    ap.add_argument("--pano", type=int, nargs=2, default=(4096, 2048))
    ap.add_argument("--batch", type=int, default=100)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-profile", action="store_true", help="skip the rocprofv3 runs")
    ap.add_argument("--commit", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "recon_timing.txt"))
    a = ap.parse_args()
    if a.step == "new":
        return step_new(a)
    if a.step == "window":
        return step_window(a)

    from cmax_slam_amd import _lib
    assert _lib.lib().cmx_device_count() > 0, "no GPU visible: this tool measures on the device only"
    commit = a.commit
    if not commit:
        try:
            commit = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], stderr=subprocess.DEVNULL).decode().strip()
        except Exception:
            commit = "unknown"
    new = child(a, "new")  # (a timing child that dies ends the run: ChildDied propagates, nothing further is started)
    old = child(a, "window")
    n = new["events"]
    L = ["whole-trajectory reconstruction: cmx_backend_recon_* vs windows of <= %d segments through the window ABI" % SEG,
         "commit: %s    %d events, %dx%d sensor, %dx%d panorama, linear spline with %d knots, batch %d, rate 1" %
         (commit, n, a.sensor[0], a.sensor[1], a.pano[0], a.pano[1], new["K"], a.batch),
         "median of %d runs after %d warm-up runs; host clock around synchronous calls; the plane is in host memory at the end" % (a.reps, a.warmup),
         "",
         "%-66s %10s %14s" % ("route", "ms", "events/s")]
    for how, label in (("host", "new, events from host arrays: begin + add + get"), ("store", "new, events from the store: begin + add_from + get")):
        L.append("%-66s %10.2f %14.3e" % (label, 1e3 * new[how]["whole_s"], n / new[how]["whole_s"]))
        L.append("%-66s %10.2f %14.3e" % ("    of which the add call", 1e3 * new[how]["add_s"], n / new[how]["add_s"]))
    for how, call in (("host", "set_window on host arrays"), ("store", "set_window_from the store")):
        L.append("%-66s %10.2f %14.3e" % ("window route: %d x (%s, eval, 2 get_plane, add)" % (old["windows"], call),
                                          1e3 * old[how]["whole_s"], n / old[how]["whole_s"]))
    L.append("")
    for how in ("host", "store"):  # like for like: the same source of events on both sides
        L.append("window route / new, both from %s: %.2f x" % ("host arrays" if how == "host" else "the store", old[how]["whole_s"] / new[how]["whole_s"]))
    slower = [h for h in ("host", "store") if new[h]["whole_s"] > old[h]["whole_s"]]
    L.append("new path slower than the window route: %s" % (", ".join(slower) if slower else "no"))
    L.append("votes: new %.1f (sampled %d, inside %d), window route %.1f (its windows cut the batches elsewhere)" %
             (new["host"]["votes"], new["host"]["sampled"], new["host"]["inside"], old["host"]["votes"]))
    died = None
    if not a.no_profile and not shutil.which("rocprofv3"):
        L += ["", "rocprofv3 is not installed: no kernel trace, no counters"]
    elif not a.no_profile:
        one = ["--reps", "1", "--warmup", "0"]
        votes = 2 * new["host"]["inside"]  # two reconstructions in a profiled run
        with tempfile.TemporaryDirectory(prefix="recon_prof_") as d:
            try:
                child(a, "new", one, ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "recon", "--"])
                L += ["", "rocprofv3 --kernel-trace --stats, one host-array and one store reconstruction:"]
                rows = sorted(rows_of(d, "kernel_stats.csv"), key=lambda r: -float(r.get("TotalDurationNs", 0) or 0))
                for r in rows[:8]:
                    L.append("  %-72s calls %5s  total %10.3f ms  %6s %%" % (r.get("Name", "?")[:72], r.get("Calls", "?"),
                                                                            float(r.get("TotalDurationNs", 0) or 0) * 1e-6, r.get("Percentage", "?")))
                vote = [r for r in rows if "recon_votes" in r.get("Name", "")]
                if vote:
                    sec = sum(float(r["TotalDurationNs"]) for r in vote) * 1e-9
                    atom, hbm = votes * 16 / sec, (votes * 16 + 2 * n * (4 + 16)) / sec
                    L.append("  vote kernel: %.3f ms for %d events: %.3e events/s" % (sec * 1e3, 2 * n, 2 * n / sec))
                    L.append("    bytes: %.3e B/s of fp32 atomic adds = %.0f %% of the ~%.1f TB/s the chip retires when every lane of a wave adds to "
                             "one 256-B run; events + bearings read + atomics = %.3e B/s = %.0f %% of %.0f TB/s HBM" %
                             (atom, 100 * atom / ATOMIC_PEAK, ATOMIC_PEAK * 1e-12, hbm, 100 * hbm / HBM_PEAK, HBM_PEAK * 1e-12))
                    L.append("    lane-adds: %.3e /s.  The votes are scattered (a lane's four adds go to two panorama rows, the lanes of a wave to "
                             "unrelated pixels), so few of them can share a memory-side request; how many requests they become is what "
                             "TCC_ATOMIC_sum below counts.  AN ESTIMATE, NOT A MEASUREMENT: were every lane-add a 64-B request of its own, "
                             "this would be %.0f %% of the %.1e 64-B requests/s behind that coalesced byte rate" %
                             (atom / 4, 100 * (atom / 4) / (ATOMIC_PEAK / 64), ATOMIC_PEAK / 64))
            except ChildDied as e:
                died = str(e).splitlines()[0]
            except Exception as e:  # clean exit, unreadable output: the timing above stands on its own
                L += ["", "rocprofv3 kernel trace: not readable (%s)" % str(e).splitlines()[0]]
        for grp in ("SQ_WAVES SQ_BUSY_CYCLES SQ_WAVE_CYCLES GRBM_GUI_ACTIVE", "SQ_INSTS_VALU SQ_INSTS_VMEM_RD SQ_INSTS_SALU SQ_INSTS_LDS",
                    "SQ_WAIT_INST_ANY SQ_WAIT_ANY SQ_ACTIVE_INST_VALU SQ_ACTIVE_INST_ANY", "TCC_HIT_sum TCC_MISS_sum TCC_REQ_sum",
                    "TCC_ATOMIC_sum TCC_READ_sum TCC_WRITE_sum TCC_EA0_ATOMIC_sum"):
            if died:
                break
            with tempfile.TemporaryDirectory(prefix="recon_pmc_") as d:
                try:
                    child(a, "new", one, ["rocprofv3", "--pmc"] + grp.split() + ["--output-format", "csv", "-d", d, "-o", "recon", "--"], limit=240)
                    acc = {}
                    for r in rows_of(d, "counter_collection.csv"):
                        if "recon_votes" in r.get("Kernel_Name", ""):
                            acc[r["Counter_Name"]] = acc.get(r["Counter_Name"], 0.0) + float(r["Counter_Value"])
                    L.append("PMC (a run of its own), recon_votes launches summed: " + ", ".join("%s %.4g" % kv for kv in sorted(acc.items())))
                    if acc.get("TCC_ATOMIC_sum"):
                        L.append("    TCC_ATOMIC_sum / lane-adds (%d events that voted x 4) = %.3f atomic requests at the L2 per lane-add" %
                                 (votes, acc["TCC_ATOMIC_sum"] / (4.0 * votes)))
                except ChildDied as e:
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
