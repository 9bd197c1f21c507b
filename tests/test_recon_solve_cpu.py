"""CPU: the frozen head and the native whole-trajectory solve (cmx_backend_recon_freeze_head / _frozen_info / _solve, and the
diagnostic cmx_diag_recon_solve_counts) are in the built library, the headers and the Python binding table with the argument types the
header states; each refuses a NULL handle before anything touches the device; the evaluator has the methods; and the prefix rule that
decides which batches are frozen (frozen_prefix, cmx_ingest.hpp) agrees with a brute-force loop under the address and
undefined-behaviour sanitizers (tests/frozen_prefix_host.cpp, a program of its own).  Needs no GPU."""
import ctypes as C
import inspect
import os
import re
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_STATE = 5

c_dp, c_i64p = C.POINTER(C.c_double), C.POINTER(C.c_int64)
NEW_SYMBOLS = {
    "cmx_backend_recon_freeze_head": (C.c_int, [C.c_void_p, C.c_int]),
    "cmx_backend_recon_frozen_info": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), c_i64p, c_i64p]),
    "cmx_backend_recon_solve": (C.c_int, [C.c_void_p, c_dp, C.c_int, C.c_int, C.c_double, C.c_int, C.c_double, C.c_double, C.c_double,
                                          C.c_double, C.c_int, C.c_void_p]),
    "cmx_diag_recon_solve_counts": (C.c_int, [C.c_void_p, c_i64p, c_i64p]),
}
# the headers' declarations, white space folded and comments dropped
HEADER_DECLS = {
    "cmx_backend_recon_freeze_head": "int cmx_backend_recon_freeze_head(cmx_ctx *ctx, int num_fixed);",
    "cmx_backend_recon_frozen_info": "int cmx_backend_recon_frozen_info(cmx_ctx *ctx, int *num_fixed, int64_t *frozen_batches, "
                                     "int64_t *frozen_sampled);",
    "cmx_backend_recon_solve": "int cmx_backend_recon_solve(cmx_ctx *ctx, double *knots_xyzw, int num_fixed, int freeze_head, "
                               "double blur_sigma, int contrast_measure, double step_size, double tol, double epsabs_grad, "
                               "double tolfun, int max_iterations, cmx_solve_report *report);",
    "cmx_diag_recon_solve_counts": "int cmx_diag_recon_solve_counts(cmx_ctx *ctx, int64_t *evaluations, int64_t *host_waits);",
}
NEW_METHODS = ["reconstruct_freeze_head", "reconstruct_frozen_info", "reconstruct_solve", "reconstruct_solve_counts"]


def _folded(path):
    with open(path) as f:
        text = " ".join(re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S).split())
    return text.replace("( ", "(").replace(" )", ")").replace(" ,", ",")


def test_library_headers_and_binding_table_carry_the_entry_points():
    from cmax_slam_amd import _lib
    assert os.path.exists(_lib.SO_PATH)
    with open(_lib.SO_PATH, "rb") as f:  # (symbol table only: the library is not initialised, no device is needed)
        blob = f.read()
    host, diag = _folded(os.path.join(ROOT, "include", "cmax_hip.h")), _folded(os.path.join(ROOT, "include", "cmax_hip_diag.h"))
    for name, sig in NEW_SYMBOLS.items():
        assert name.encode() + b"\0" in blob, name
        assert HEADER_DECLS[name] in (diag if name.startswith("cmx_diag") else host), name
        assert name in _lib.SYMBOLS, name
        restype, argtypes = _lib.SYMBOLS[name]
        assert restype is sig[0] and list(argtypes) == sig[1], name
    assert "#define CMX_ABI_VERSION 6" in host
    # the solve is declared where its report type is known: a C host includes the header as it is
    assert host.index("} cmx_solve_report;") < host.index("int cmx_backend_recon_solve(")


def test_a_null_handle_is_a_state_error():
    from cmax_slam_amd import _lib
    L = C.CDLL(_lib.SO_PATH)  # (loaded, not initialised: the front door refuses a NULL handle before any HIP call)
    for name, (restype, argtypes) in NEW_SYMBOLS.items():
        fn = getattr(L, name)
        fn.restype, fn.argtypes = restype, argtypes
    assert _lib.ERR_STATE == ERR_STATE
    k = (C.c_double * 8)(0, 0, 0, 1, 0, 0, 0, 1)
    assert L.cmx_backend_recon_freeze_head(None, 1) == ERR_STATE
    assert L.cmx_backend_recon_frozen_info(None, None, None, None) == ERR_STATE
    assert L.cmx_backend_recon_solve(None, k, 1, 0, 1.0, 0, 0.1, 0.1, 1e-4, 1e-4, 50, None) == ERR_STATE
    assert L.cmx_diag_recon_solve_counts(None, None, None) == ERR_STATE


def test_evaluator_has_the_methods():
    from cmax_slam_amd import evaluator
    for name in NEW_METHODS:
        assert callable(getattr(evaluator.BackendEvaluator, name, None)), name
    p = inspect.signature(evaluator.BackendEvaluator.reconstruct_solve).parameters
    assert list(p)[1:6] == ["knots", "num_fixed", "sigma", "measure", "freeze_head"]
    assert [p[k].default for k in ("sigma", "measure", "freeze_head")] == [1.0, evaluator.VARIANCE, False]


def test_the_prefix_rule_against_brute_force(tmp_path):
    """frozen_prefix / batch_is_frozen alone, under the address and undefined-behaviour sanitizers, run directly:
    orders 2 and 4, num_fixed in {0, order - 1, order, K - 1}, a batch time exactly on a knot boundary, a recording that ends
    before the first free knot's support, one batch, zero batches (tests/frozen_prefix_host.cpp)."""
    exe = str(tmp_path / "frozen_prefix_host")
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "frozen_prefix_host.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and r.stdout.startswith("ok ")
