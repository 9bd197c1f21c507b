#!/usr/bin/env python3
"""Timing of the event-store selection (cmx_events_select_device, cmx_events_pixel_counts_device)
-> profiles/events_select_timing.txt.

tools/time_recon.py's large configuration -- 20M events over 20 s in an event store, 1280x720 sensor, 4096x2048 panorama, linear
spline with 401 knots, batch 100 -- with the leave-one-out scores of score_from_device at sigma 1 as the criterion and the threshold
at the quantile that keeps about 0.1 / 0.5 / 0.9 of the events (1.0: min_score = -inf).  Per share, medians of --reps after --warmup:
    (a) kernels   the three kernels of one call (mark + scan + scatter): their mean durations from `rocprofv3 --kernel-trace --stats`
                  around a child process that makes the same calls (one child per share; "n/a" when the profiler is not there)
    (b) call      host clock around select_device: the kernels, the 8-byte read of the total, the timestamps' device-to-host copy
                  into the host mirror
    (c) floor     in the same run, a plain device-to-device copy of the bytes the call stores (kept x 12; torch's copy_ of a byte
                  tensor, one hipMemcpyAsync) + synchronize
    (d) host      in the same run, the route a host takes without the call: score_from into host arrays, the numpy mask, the cut
                  copies of x, y, t, push into an empty store
and pixel_counts_device over the 20M events, uniform and with two hot pixels that hold 2 % of the events each.  Needs a GPU."""
import argparse
import glob
import os
import shutil
import signal
import sqlite3
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402

import time_recon as tr  # noqa: E402  (the stream of the large configuration)
from time_recon_warp import median_ms  # noqa: E402

SHARES = (0.1, 0.5, 0.9, 1.0)
KERNELS = ("select_mark_kernel", "select_scan_kernel", "select_scatter_kernel")


def scored(a):
    """(x, y, t, src store, device scores, device flags, host scores) of the configuration"""
    import torch
    from cmax_slam_amd import evaluator
    x, y, t, knots, start_ns, dt_ns, lut = tr.make_inputs(a)
    n = len(x)
    be = evaluator.BackendEvaluator(a.sensor[0], a.sensor[1], lut, a.pano[0], a.pano[1])
    src = evaluator.EventStore(a.sensor[0], a.sensor[1], n)
    src.push(x, y, t)
    be.reconstruct_begin(2, knots, start_ns, dt_ns, a.batch, 1)
    be.reconstruct_add_from(src, 0, n)
    be.reconstruct_score_open(1.0)
    d_s = torch.empty(n, dtype=torch.float32, device="cuda")
    d_f = torch.empty(n, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    be.reconstruct_score_from(src, 0, n, loo=True, out=(d_s, d_f))
    return x, y, t, be, src, d_s, d_f, d_s.cpu().numpy()


def threshold(s, share):
    return float("-inf") if share >= 1.0 else float(np.quantile(s, 1.0 - share))


def child(a):
    """the calls of (b) alone, for the profiler"""
    from cmax_slam_amd import evaluator
    x, y, t, be, src, d_s, d_f, s = scored(a)
    n = len(x)
    dst = evaluator.EventStore(a.sensor[0], a.sensor[1], n)
    thr = threshold(s, a.child_share)
    for _ in range(a.warmup + a.reps):
        dst.drop_before(dst.end)
        dst.select(src, 0, n, score=d_s, min_score=thr)
    return 0


def kernel_ms(a, share, limit=420):
    """mean duration of the three kernels over the child's calls, ms each, or None when there is no profiler.  A child that ends
    with a non-zero status or runs into its limit raises time_recon.ChildDied: nothing more is started on the GPU after it."""
    exe = shutil.which("rocprofv3")
    if not exe:
        return None
    d = tempfile.mkdtemp(prefix="selprof_")
    try:
        cmd = [exe, "--kernel-trace", "--stats", "-d", d, "-o", "trace", "--", sys.executable, os.path.abspath(__file__), "--child-share",
               str(share), "--events", str(a.events), "--seconds", str(a.seconds), "--sensor", str(a.sensor[0]), str(a.sensor[1]),
               "--pano", str(a.pano[0]), str(a.pano[1]), "--batch", str(a.batch), "--reps", str(a.reps), "--warmup", str(a.warmup)]
        # a session (hence a process group) of its own: the process that holds the GPU is the profiler's child, and the limit has
        # to end it too (tools/time_recon.py's child())
        p = subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, cwd=ROOT, start_new_session=True)
        try:
            raw, _ = p.communicate(timeout=limit)
        except subprocess.TimeoutExpired:
            try:
                os.killpg(p.pid, signal.SIGKILL)
            except ProcessLookupError:
                pass
            p.communicate()
            raise tr.ChildDied("the profiled child at share %g was killed at its limit of %d s" % (share, limit))
        if p.returncode != 0:
            raise tr.ChildDied("the profiled child at share %g ended with status %d:\n%s" % (share, p.returncode, raw.decode(errors="replace")[-2000:]))
        out = {}
        for db in glob.glob(os.path.join(d, "**", "*_results.db"), recursive=True):
            con = sqlite3.connect(db)
            try:
                rows = con.execute("select name, total_calls, average from top_kernels").fetchall()
            except sqlite3.Error:  # (a profiler whose output has another layout: no kernel column, the run itself was fine)
                rows = []
            finally:
                con.close()
            for name, calls, avg in rows:
                for k in KERNELS:
                    if k in name:
                        out[k] = (float(avg) / 1e3, int(calls))  # (the view is in microseconds)
        return out or None
    finally:
        shutil.rmtree(d, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--events", type=int, default=20_000_000)
    ap.add_argument("--seconds", type=float, default=20.0)
    ap.add_argument("--sensor", type=int, nargs=2, default=(1280, 720))
    ap.add_argument("--pano", type=int, nargs=2, default=(4096, 2048))
    ap.add_argument("--batch", type=int, default=100)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-kernel-trace", action="store_true")
    ap.add_argument("--child-share", type=float, default=None, help=argparse.SUPPRESS)
    ap.add_argument("--commit", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "events_select_timing.txt"))
    a = ap.parse_args()
    if a.child_share is not None:
        return child(a)
    # (a) first: the children run one after the other while this process has not opened the device; the first one that dies ends the
    # tool (ChildDied) before anything else is started
    kern = {}
    for sh in SHARES:
        kern[sh] = None if a.no_kernel_trace else kernel_ms(a, sh)

    import torch
    from cmax_slam_amd import _lib, evaluator
    L = _lib.lib()
    assert L.cmx_device_count() > 0, "no GPU visible: this tool measures on the device only"
    commit = a.commit
    if not commit:
        try:
            commit = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], stderr=subprocess.DEVNULL).decode().strip()
        except Exception:
            commit = "unknown"
    x, y, t, be, src, d_s, d_f, s = scored(a)
    n = len(x)
    W, H = a.sensor
    dst = evaluator.EventStore(W, H, n)
    host_dst = evaluator.EventStore(W, H, n)
    sc, fl = np.zeros(n, np.float32), np.zeros(n, np.uint8)  # (touched: no first-touch page faults inside the timed call)
    rows = []
    for share in SHARES:
        thr = threshold(s, share)
        r = {"share": share, "thr": thr}

        def call():
            r["kept"] = dst.select(src, 0, n, score=d_s, min_score=thr)

        def timed(fn, before):
            v = []
            for i in range(a.warmup + a.reps):
                before()
                t0 = time.perf_counter()
                fn()
                if i >= a.warmup:
                    v.append(1e3 * (time.perf_counter() - t0))
            return float(np.median(v)), min(v)

        r["call"] = timed(call, lambda: dst.drop_before(dst.end))
        nbytes = r["kept"] * 12
        a_buf = torch.empty(max(nbytes, 1), dtype=torch.uint8, device="cuda")
        b_buf = torch.empty(max(nbytes, 1), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()

        def floor():
            b_buf.copy_(a_buf)
            torch.cuda.synchronize()
        r["floor"] = median_ms(floor, a.warmup, a.reps)
        del a_buf, b_buf

        def host():
            be._ck(L.cmx_backend_recon_score_from(be._ctx, src._h, 0, n, 1, sc.ctypes.data, fl.ctypes.data))
            m = sc >= np.float32(thr)
            host_dst.push(x[m], y[m], t[m])
        r["host"] = timed(host, lambda: host_dst.drop_before(host_dst.end))
        assert host_dst.end - host_dst.begin == r["kept"], (host_dst.end - host_dst.begin, r["kept"])
        rows.append(r)
    be.reconstruct_end()

    # the histogram: uniform pixels, then two hot pixels at 2 % of the events each
    d_c = torch.empty(W * H, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    hist = [median_ms(lambda: src.pixel_counts(0, n, out=d_c), a.warmup, a.reps)]
    assert int(d_c.sum().item()) == n
    dst.close()
    host_dst.close()
    rng = np.random.default_rng(12)
    xh, yh = x.copy(), y.copy()
    at = rng.permutation(n)[:int(0.04 * n)]
    xh[at[::2]], yh[at[::2]] = 100, 100
    xh[at[1::2]], yh[at[1::2]] = W - 7, H - 9
    hot = evaluator.EventStore(W, H, n)
    hot.push(xh, yh, t)
    hist.append(median_ms(lambda: hot.pixel_counts(0, n, out=d_c), a.warmup, a.reps))
    c = d_c.cpu().numpy().reshape(H, W)
    assert int(c.sum()) == n and int(c[100, 100]) >= len(at[::2]) and int(c[H - 9, W - 7]) >= len(at[1::2])

    Ls = ["event-store selection: cmx_events_select_device, cmx_events_pixel_counts_device",
          "commit %s; %d events over %.0f s in an event store (no polarity), sensor %dx%d; scores: score_from_device, leave-one-out, sigma 1, "
          "panorama %dx%d, linear spline of %d knots, batch %d" % (commit, n, a.seconds, W, H, a.pano[0], a.pano[1], 401, a.batch),
          "ms: median (min) of %d after %d warm-up calls, host clock around synchronous calls; (a) mean kernel durations of a profiled child "
          "process making the same calls" % (a.reps, a.warmup), "",
          "share   kept        (a) kernels: mark + scan + scatter = sum        (b) whole call      (c) D2D copy of kept x 12 B   (d) host route: "
          "score_from + mask + cut + push    (a)/(c)   (b)/(d)"]
    for r in rows:
        k = kern.get(r["share"])
        if k and all(q in k for q in KERNELS):
            ks = [k[q][0] for q in KERNELS]
            ka = "%6.3f + %6.3f + %6.3f = %7.3f" % (ks[0], ks[1], ks[2], sum(ks))
            ratio = "%6.2fx" % (sum(ks) / r["floor"][0])
        else:
            ka, ratio = "n/a (no kernel trace)            ", "   n/a "
        Ls.append("%4.2f  %9d     %s          %8.3f (%.3f)     %8.3f (%.3f)             %9.3f (%.3f)                       %s   %6.3fx" %
                  (r["kept"] / n, r["kept"], ka, r["call"][0], r["call"][1], r["floor"][0], r["floor"][1], r["host"][0], r["host"][1], ratio,
                   r["call"][0] / r["host"][0]))
    Ls += ["", "bytes the kernels move per event: 4 (score) + 1/8 (ballot, written) + 1/8 (ballot, read) + share x (12 read + 12 written)",
           "pixel_counts_device over all %d events (memset of %d words + one integer atomic per event + synchronize):" % (n, W * H),
           "  uniform pixels                                  %8.3f (%.3f)" % hist[0],
           "  two hot pixels holding 2 %% of the events each   %8.3f (%.3f)" % hist[1]]
    text = "\n".join(Ls) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
