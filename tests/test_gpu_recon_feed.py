"""GPU: the one staging path under cmx_backend_recon_add*, _grad_add* and _warp* (cmx_recon_feed.cpp), with its consumers
interleaved on ONE context: votes from host arrays, an export from the store, the image pass, an export from records, the gradient
pass from the store, the results.  The internal slice size changes from round to round (1000, 4096, the default), so the two input
slots and the export's two output slots are used small, then grown, then used as one slice.

Deterministic mode, so nothing needs a tolerance: plane, counters, contrast and gradient are bit for bit those of the same calls
with no export in between (at the same slice size: the gradient's rows are summed slice by slice), and both exports have the bytes of
a fresh context's export, which does not depend on the slices at all."""
import numpy as np
import pytest

import recon_cases as rc
from cmax_slam_amd import _lib

pytestmark = pytest.mark.gpu
W, H = rc.SENSOR[:2]
SIGMA = 1.0


def make(hip, name):
    c, w = rc.CASES[name], rc.window(name)[0]
    be = hip.BackendEvaluator(W, H, w.lut, c["Wp"], c["Hp"])
    be.set_deterministic(True)
    be.reconstruct_begin(c["order"], w.knots_true, w.start_ns, w.dt_ns, c["batch"], c["rate"])
    return be


def sequence(be, name, store, exports):
    """the seven steps (exports: with steps 2 and 4); everything they return"""
    w, x, y, t = rc.window(name)
    n = len(x)
    be.reconstruct_restart(w.knots_true)
    be.reconstruct_add(x, y, t)
    from_store = be.reconstruct_warp_from(store, 0, n) if exports else None
    contrast = be.reconstruct_contrast(SIGMA, want_grad=True)
    from_records = be.reconstruct_warp_aos(_lib.dvs_events(x, y, t)) if exports else None
    be.reconstruct_grad_add_from(store, 0, n)
    grad = be.reconstruct_grad_get()
    plane, n_sampled, n_inside = be.reconstruct_get(with_counts=True)
    return dict(plane=plane, counts=(n_sampled, n_inside), contrast=contrast, grad=grad, from_store=from_store, from_records=from_records)


@pytest.mark.parametrize("name", ["B", "n65"])  # sub-sampled with a short last batch; one batch and the lone trailing event
def test_consumers_interleaved_on_one_context(hip, name):
    c = rc.CASES[name]
    _, x, y, t = rc.window(name)
    n = c["N"]
    store = hip.EventStore(W, H, n)
    store.push(x, y, t)
    fresh = make(hip, name)
    want_xy, want_fl = fresh.reconstruct_warp_from(store, 0, n)
    fresh.reconstruct_end()
    assert want_xy.shape == (n, 2) and want_fl.shape == (n,)
    assert int((want_fl & 1).sum()) == sum(len(range(b, min(b + c["batch"], n), c["rate"])) for b in range(0, n - 1, c["batch"]))
    be, plain = make(hip, name), make(hip, name)
    L = _lib.lib()
    try:
        for n_slice in (1000, 4096, 0):
            assert L.cmx_diag_set(_lib.DIAG_RECON_SLICE_EVENTS, n_slice) == 0
            got, ref = sequence(be, name, store, True), sequence(plain, name, store, False)
            assert got["counts"] == ref["counts"] and got["counts"][0] == rc.sampled(n, c["batch"], c["rate"]), n_slice
            assert got["counts"][1] > 0 and np.any(ref["grad"] != 0), n_slice  # (no empty comparison)
            assert got["plane"].tobytes() == ref["plane"].tobytes(), n_slice
            assert np.float64(got["contrast"]).tobytes() == np.float64(ref["contrast"]).tobytes(), n_slice
            assert got["grad"].tobytes() == ref["grad"].tobytes(), n_slice
            for how in ("from_store", "from_records"):
                xy, fl = got[how]
                assert xy.dtype == want_xy.dtype and xy.tobytes() == want_xy.tobytes() and fl.tobytes() == want_fl.tobytes(), (n_slice, how)
    finally:
        assert L.cmx_diag_set(_lib.DIAG_RECON_SLICE_EVENTS, 0) == 0
    be.reconstruct_end()
    plain.reconstruct_end()
    store.close()
