"""CPU: the built library, the header and the Python binding table carry the four entry points of the bound whole-trajectory
evaluation (cmx_backend_recon_bind_from / _unbind / _eval_bound / _bound_info) with the argument types the header states, each of
them refuses a NULL handle before anything touches the device, the evaluator has the methods -- and the 48 x 40 panorama of
tests/test_gpu_recon_bound.py is a fair comparison on the CPU oracle: it votes, and its gradient is not zero.  Needs no GPU."""
import ctypes as C
import inspect
import os
import re
import shutil
import subprocess

import numpy as np

import recon_cases as rc
from test_gpu_recon_bound import SMALL, small_window

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_STATE = 5

c_dp, c_i64p = C.POINTER(C.c_double), C.POINTER(C.c_int64)
NEW_SYMBOLS = {
    "cmx_backend_recon_bind_from": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64]),
    "cmx_backend_recon_unbind": (C.c_int, [C.c_void_p]),
    "cmx_backend_recon_eval_bound": (C.c_int, [C.c_void_p, c_dp, C.c_double, C.c_int, c_dp, c_dp]),
    "cmx_backend_recon_bound_info": (C.c_int, [C.c_void_p, c_i64p, c_i64p, c_i64p, c_dp]),
}
# the header's declarations, white space folded and comments dropped
HEADER_DECLS = {
    "cmx_backend_recon_bind_from": "int cmx_backend_recon_bind_from(cmx_ctx *ctx, const cmx_events *ev, int64_t first, int64_t count);",
    "cmx_backend_recon_unbind": "int cmx_backend_recon_unbind(cmx_ctx *ctx);",
    "cmx_backend_recon_eval_bound": "int cmx_backend_recon_eval_bound(cmx_ctx *ctx, const double *knots_xyzw, double blur_sigma, "
                                    "int contrast_measure, double *contrast, double *grad);",
    "cmx_backend_recon_bound_info": "int cmx_backend_recon_bound_info(cmx_ctx *ctx, int64_t *n_events, int64_t *n_sampled, "
                                    "int64_t *sorts, double *fallback_frac);",
}
NEW_METHODS = ["reconstruct_bind", "reconstruct_unbind", "reconstruct_eval_bound", "reconstruct_bound_info"]


def test_library_header_and_binding_table_carry_the_entry_points():
    from cmax_slam_amd import _lib
    assert os.path.exists(_lib.SO_PATH)
    with open(_lib.SO_PATH, "rb") as f:  # (symbol table only: the library is not initialised, no device is needed)
        blob = f.read()
    with open(os.path.join(ROOT, "include", "cmax_hip.h")) as f:
        header = " ".join(re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S).split())
    header = header.replace("( ", "(").replace(" )", ")").replace(" ,", ",")
    for name, sig in NEW_SYMBOLS.items():
        assert name.encode() + b"\0" in blob, name
        assert HEADER_DECLS[name] in header, name
        assert name in _lib.SYMBOLS, name
        restype, argtypes = _lib.SYMBOLS[name]
        assert restype is sig[0] and list(argtypes) == sig[1], name
    assert "#define CMX_ABI_VERSION 6" in header


def test_a_null_handle_is_a_state_error():
    from cmax_slam_amd import _lib
    L = C.CDLL(_lib.SO_PATH)  # (loaded, not initialised: recon_enter refuses a NULL handle before any HIP call)
    for name, (restype, argtypes) in NEW_SYMBOLS.items():
        fn = getattr(L, name)
        fn.restype, fn.argtypes = restype, argtypes
    assert _lib.ERR_STATE == ERR_STATE
    out, g = C.c_double(), (C.c_double * 3)()
    assert L.cmx_backend_recon_bind_from(None, None, 0, 0) == ERR_STATE
    assert L.cmx_backend_recon_unbind(None) == ERR_STATE
    assert L.cmx_backend_recon_eval_bound(None, None, 1.0, 0, C.byref(out), g) == ERR_STATE
    assert L.cmx_backend_recon_bound_info(None, None, None, None, None) == ERR_STATE


def test_evaluator_has_the_methods():
    from cmax_slam_amd import evaluator
    for name in NEW_METHODS:
        assert callable(getattr(evaluator.BackendEvaluator, name, None)), name
    p = inspect.signature(evaluator.BackendEvaluator.reconstruct_refine).parameters
    assert p["bind"].default is False
    p = inspect.signature(evaluator.BackendEvaluator.reconstruct_eval_bound).parameters
    assert [p[k].default for k in ("knots", "sigma", "want_grad")] == [None, 1.0, True]


def test_host_arithmetic_of_a_binding(tmp_path):
    """plan_chunks / slice_at (cmx_ingest.hpp) alone, under the address and undefined-behaviour sanitizers: the slices of a pass
    tile the packed events and the events handed in, the chunk table's bound holds for every distribution build_chunks can meet,
    the front end's divisor gives the window path's formula, nothing overflows an int at the limits (tests/bound_plan_host.cpp)."""
    exe = str(tmp_path / "bound_plan_host")
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "bound_plan_host.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and r.stdout.startswith("ok ")


def test_the_small_panorama_is_a_fair_comparison(oracle):
    w, x, y, t, q = small_window()
    c = rc.CASES["batch3"]
    Wf, Hf = rc.SENSOR[:2]
    K = len(q)
    b = oracle.Backend(Wf, Hf, w.lut, SMALL[0], SMALL[1], c["order"], c["batch"], c["rate"], sigma=0.0)
    b.set_window(x, y, t, q, w.start_ns, w.dt_ns, K, 2 ** 62)
    plane = b.accumulate_raw(np.zeros(0))[0]
    votes = float(plane.sum(dtype=np.float64))
    b = oracle.Backend(Wf, Hf, w.lut, SMALL[0], SMALL[1], c["order"], c["batch"], c["rate"], sigma=1.0, measure=0)
    b.set_window(x, y, t, q, w.start_ns, w.dt_ns, 0, 2 ** 62)
    con, g = b.eval(np.zeros(3 * K), True)
    print("48 x 40: %.1f of %d sampled events vote, contrast %.6g, |g|max %.4g" %
          (votes, rc.sampled(c["N"], c["batch"], c["rate"]), con, np.abs(g).max()))
    assert plane.shape == (SMALL[1], SMALL[0])
    assert votes > 0.5 * rc.sampled(c["N"], c["batch"], c["rate"])  # (every vote adds weights that sum to one)
    assert con > 0 and np.abs(g).max() > 0
