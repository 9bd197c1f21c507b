"""CPU: the comparisons of tests/test_gpu_recon_grad.py are not empty, the oracle they are held against is itself accurate enough for
the project's tolerance at the (case, sigma) pairs they use, the properties the whole-trajectory gradient's contract quotes hold in
the oracle -- and the built library and the Python evaluator carry the new entry points.  Needs no GPU."""
import ctypes
import os

import numpy as np
import pytest

import recon_cases as rc
import recon_grad_cases as rg
from util import rel_scalar, rel_vec

NEW_SYMBOLS = ["cmx_backend_recon_restart", "cmx_backend_recon_contrast", "cmx_backend_recon_grad_add", "cmx_backend_recon_grad_add_aos",
               "cmx_backend_recon_grad_add_from", "cmx_backend_recon_grad_get", "cmx_backend_recon_eval_from"]
NEW_METHODS = ["reconstruct_restart", "reconstruct_contrast", "reconstruct_grad_add", "reconstruct_grad_add_aos",
               "reconstruct_grad_add_from", "reconstruct_grad_get", "reconstruct_eval", "reconstruct_refine"]


def test_library_exports_the_new_entry_points():
    from cmax_slam_amd import _lib
    assert os.path.exists(_lib.SO_PATH)
    # (symbol table only: the library is not initialised, no device is needed)
    with open(_lib.SO_PATH, "rb") as f:
        blob = f.read()
    for name in NEW_SYMBOLS:
        assert name.encode() + b"\0" in blob, name
        assert name in _lib.SYMBOLS, name
    L = ctypes.CDLL(_lib.SO_PATH)
    for name in NEW_SYMBOLS:
        assert getattr(L, name) is not None


def test_evaluator_has_the_new_methods():
    from cmax_slam_amd import evaluator
    for name in NEW_METHODS:
        assert callable(getattr(evaluator.BackendEvaluator, name, None)), name


@pytest.mark.parametrize("name", rg.SIGMA1)
def test_no_comparison_is_empty(oracle, name):
    c, g = rg.oracle_ref(oracle, name, 1.0, 0)
    K = rc.CASES[name]["K"]
    assert g.shape == (3 * K,)
    assert c > 0
    print("%s: contrast %.6g, |g|max %.4g" % (name, c, np.abs(g).max()))
    assert np.abs(g).max() > 0
    if name in ("A", "B"):  # every knot of the two long splines carries gradient
        assert (np.abs(g.reshape(K, 3)).max(axis=1) > 0).all()


@pytest.mark.parametrize("name,sigma", [(n, 1.0) for n in rg.SIGMA1] + [(n, s) for n in rg.SIGMA02 for s in (0.0, 2.0)])
def test_oracle_is_within_3e_6_of_its_fp64_build(oracle, name, sigma):
    _, x, y, t = rc.window(name)
    c, g = rg.oracle_ref(oracle, name, sigma, 0)
    ce, ge = rg.oracle_eval(oracle, name, x, y, t, rg.point(name), sigma, 0, exact=True)
    print("%s sigma %g: contrast %.2e, gradient %.2e" % (name, sigma, rel_scalar(c, ce), rel_vec(g, ge)))
    assert rel_scalar(c, ce) < 3e-6
    assert rel_vec(g, ge) < 3e-6


def test_side_slice_and_offset_properties(oracle):
    """what the contract quotes: the old / new side changes no bit; num_fixed = f is the slice [3f:]; a spline embedded at an offset
    in a longer identity trajectory has exact zeros in front and bitwise the same values behind"""
    name = "B"
    cfg, (w, x, y, t) = rc.CASES[name], rc.window(name)
    q = rg.point(name)
    c0, g0 = rg.oracle_ref(oracle, name, 1.0, 0)
    c1, g1 = rg.oracle_eval(oracle, name, x, y, t, q, side=-2 ** 62)  # every event "new"
    assert c1 == c0 and g1.tobytes() == g0.tobytes()
    f = 5
    c2, g2 = rg.oracle_eval(oracle, name, x, y, t, q, num_fixed=f)
    assert c2 == c0 and g2.tobytes() == g0[3 * f:].tobytes()
    off = 33
    long = np.zeros((cfg["K"] + off, 4))
    long[:, 3] = 1.0
    long[off:] = q
    c3, g3 = rg.oracle_eval(oracle, name, x, y, t, long, start_ns=w.start_ns - off * w.dt_ns)
    assert c3 == c0
    assert not g3[:3 * off].any()
    assert g3[3 * off:].tobytes() == g0.tobytes()
