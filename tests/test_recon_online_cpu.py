"""CPU: the growing whole-trajectory binding (cmx_backend_recon_extend / _bind_append_from / _advance_head / _release_head /
_online_info, and CMX_RECON_KEEP_HEAD of cmx_backend_recon_solve) is in the built library, the header and the Python binding table
with the argument types the header states; each refuses a NULL handle before anything touches the device; the evaluator has the
methods; the planner of an append (plan_append, cmx_ingest.hpp) agrees with a brute-force plan of the concatenation under the
address and undefined-behaviour sanitizers (tests/append_plan_host.cpp, a program of its own); and the schedules the GPU tests run
(tests/recon_online_cases.py) are no empty comparisons.  Needs no GPU."""
import ctypes as C
import inspect
import os
import re
import shutil
import subprocess

import numpy as np

import recon_cases as rc
import recon_online_cases as ro

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_STATE = 5

c_dp, c_i64p = C.POINTER(C.c_double), C.POINTER(C.c_int64)
NEW_SYMBOLS = {
    "cmx_backend_recon_extend": (C.c_int, [C.c_void_p, C.c_int, c_dp]),
    "cmx_backend_recon_bind_append_from": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64]),
    "cmx_backend_recon_advance_head": (C.c_int, [C.c_void_p, C.c_int]),
    "cmx_backend_recon_release_head": (C.c_int, [C.c_void_p]),
    "cmx_backend_recon_online_info": (C.c_int, [C.c_void_p, c_i64p, c_i64p, c_i64p, c_i64p]),
}
HEADER_DECLS = {
    "cmx_backend_recon_extend": "int cmx_backend_recon_extend(cmx_ctx *ctx, int K_new, const double *knots_xyzw);",
    "cmx_backend_recon_bind_append_from": "int cmx_backend_recon_bind_append_from(cmx_ctx *ctx, const cmx_events *ev, int64_t first, "
                                          "int64_t count);",
    "cmx_backend_recon_advance_head": "int cmx_backend_recon_advance_head(cmx_ctx *ctx, int num_fixed_new);",
    "cmx_backend_recon_release_head": "int cmx_backend_recon_release_head(cmx_ctx *ctx);",
    "cmx_backend_recon_online_info": "int cmx_backend_recon_online_info(cmx_ctx *ctx, int64_t *released_batches, int64_t *released_events, "
                                     "int64_t *released_sampled, int64_t *resident_sampled);",
}
NEW_METHODS = ["reconstruct_extend", "reconstruct_bind_append", "reconstruct_advance_head", "reconstruct_release_head",
               "reconstruct_online_info"]


def _folded(path):
    with open(path) as f:
        text = " ".join(re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S).split())
    return text.replace("( ", "(").replace(" )", ")").replace(" ,", ",")


def test_library_header_and_binding_table_carry_the_entry_points():
    from cmax_slam_amd import _lib
    assert os.path.exists(_lib.SO_PATH)
    with open(_lib.SO_PATH, "rb") as f:  # (symbol table only: the library is not initialised, no device is needed)
        blob = f.read()
    host = _folded(os.path.join(ROOT, "include", "cmax_hip.h"))
    for name, sig in NEW_SYMBOLS.items():
        assert name.encode() + b"\0" in blob, name
        assert HEADER_DECLS[name] in host, name
        assert name in _lib.SYMBOLS, name
        restype, argtypes = _lib.SYMBOLS[name]
        assert restype is sig[0] and list(argtypes) == sig[1], name
    assert "#define CMX_ABI_VERSION 6" in host  # added without a bump
    assert "#define CMX_RECON_KEEP_HEAD 2" in host and _lib.RECON_KEEP_HEAD == 2


def test_a_null_handle_is_a_state_error():
    from cmax_slam_amd import _lib
    L = C.CDLL(_lib.SO_PATH)  # (loaded, not initialised: the front door refuses a NULL handle before any HIP call)
    for name, (restype, argtypes) in NEW_SYMBOLS.items():
        fn = getattr(L, name)
        fn.restype, fn.argtypes = restype, argtypes
    assert _lib.ERR_STATE == ERR_STATE
    k = (C.c_double * 8)(0, 0, 0, 1, 0, 0, 0, 1)
    assert L.cmx_backend_recon_extend(None, 2, k) == ERR_STATE
    assert L.cmx_backend_recon_bind_append_from(None, None, 0, 0) == ERR_STATE
    assert L.cmx_backend_recon_advance_head(None, 1) == ERR_STATE
    assert L.cmx_backend_recon_release_head(None) == ERR_STATE
    assert L.cmx_backend_recon_online_info(None, None, None, None, None) == ERR_STATE
    L.cmx_backend_recon_solve.restype = C.c_int
    L.cmx_backend_recon_solve.argtypes = [C.c_void_p, c_dp, C.c_int, C.c_int, C.c_double, C.c_int, C.c_double, C.c_double, C.c_double,
                                          C.c_double, C.c_int, C.c_void_p]
    assert L.cmx_backend_recon_solve(None, k, 1, 2, 1.0, 0, 0.1, 0.1, 1e-4, 1e-4, 50, None) == ERR_STATE


def test_evaluator_has_the_methods():
    from cmax_slam_amd import evaluator
    for name in NEW_METHODS:
        assert callable(getattr(evaluator.BackendEvaluator, name, None)), name
    p = inspect.signature(evaluator.BackendEvaluator.reconstruct_bind_append).parameters
    assert list(p)[1:] == ["store", "first", "count"]
    assert list(inspect.signature(evaluator.BackendEvaluator.reconstruct_extend).parameters)[1:] == ["knots_xyzw"]
    assert "keep" in inspect.getsource(evaluator.BackendEvaluator.reconstruct_solve)


def test_the_append_planner_against_brute_force(tmp_path):
    """plan_append / open_tail_from alone, under the address and undefined-behaviour sanitizers, run directly: B in {1, 3, 64,
    5000}, rates 1 to 3, appends of 0, 1, B - 1, B and B + 1 events behind bindings of 0, 1, 2, B - 1, B, B + 1 and 2 B + 1
    (tests/append_plan_host.cpp)."""
    exe = str(tmp_path / "append_plan_host")
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "append_plan_host.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and r.stdout.startswith("ok ")


# what the schedules were chosen for: (events, frozen batches, batches) per step
EXPECT = {
    "A": [(22_671, 106, 227), (41_343, 289, 414), (60_007, 476, 601)],
    "B": [(None, 74, 197), (None, 197, 331), (None, 364, 469)],
}


def test_the_schedules_are_no_empty_comparisons():
    for name, steps in ro.SCHEDULES.items():
        c = rc.CASES[name]
        assert steps[-1][0] == c["K"] and ro.cut(name, c["K"]) == c["N"]  # the last step holds the whole stream
        prev_n, prev_fb, prev_nf, prev_K = 0, 0, 0, 0
        for i, (K, nf) in enumerate(steps):
            n = ro.cut(name, K)
            fb, nb = ro.frozen_batches(name, n, K, nf)
            print("%s step %d: K %d num_fixed %d: %d events, %d / %d batches frozen" % (name, i, K, nf, n, fb, nb))
            assert K > prev_K and prev_nf <= nf < K and n > prev_n
            if c["batch"] > 1 and i + 1 < len(steps):  # (the cuts between steps; the last one is the end of the stream)
                assert n % c["batch"] != 0, "the cut falls on a batch boundary"
            assert fb < nb, "no active batch"
            if (name, i) in ro.NOTHING_NEW:
                assert fb == prev_fb
            else:
                assert fb > prev_fb, "nothing newly frozen"
            # the batches frozen so far were closed ones when the next range was appended: no append meets a frozen open batch
            assert prev_fb <= prev_n // c["batch"]
            if name in EXPECT:
                en, efb, enb = EXPECT[name][i]
                assert (fb, nb) == (efb, enb) and (en is None or en == n)
            # the knots of the step: the settled ones keep their bytes, the others move
            q = ro.knots(name)[i]
            assert q.shape == (K, 4)
            if i:
                q0 = ro.knots(name)[i - 1]
                assert q[:prev_nf].tobytes() == q0[:prev_nf].tobytes() and not np.array_equal(q[prev_nf:prev_K], q0[prev_nf:])
            prev_n, prev_fb, prev_nf, prev_K = n, fb, nf, K
    # batch3's first cut leaves a lone trailing event; with batch 1 every append re-opens one
    assert ro.cut("batch3", 6) % 3 == 1 and ro.cut("batch3", 6) == 5332
