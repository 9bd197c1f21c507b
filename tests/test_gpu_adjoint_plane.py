"""-m gpu: Jt, the plane every gradient gather reads, per pixel against fp64 operators (tests/dense_image_ops.py).

Every form that produces Jt -- the fused tile pass, image_adjoint2<4>, image_adjoint2g, the four-pass image_adjoint_kernel<4 | -1>,
the Sobel pass, their tile-list variants, and the same launcher on the whole-trajectory plane -- has its own halo arithmetic and its
own REFLECT_101 fold of the border taps.  The other adjoint tests see Jt through a gradient summed over all events, which dilutes an
error confined to one tile column, one border row or one corner; here the plane itself is read back (cmx_diag_get_adjoint_plane)
after one evaluation on a fresh context and compared with Gy^T (Gy A Gx^T) Gx, A being the forward plane as the host knows it:

* front end: integer-pixel events at omega = 0 (dense_image_ops.exact_packet), A by counting, checked equal to get_iwe(blur = 0);
* back-end window: A = fl32(IG * (float) alpha + (IL_old + IL_new)) from get_plane, get_alpha and the map handed in -- the kernels'
  own expression, op for op;
* whole trajectory: A = reconstruct_get's plane.

The bound is made on the CPU from the reference side alone: 8 max(e32, 2^-24) max |Jt_ref|, e32 the error of the same passes run in
fp32 on the host (dense_image_ops.bound); dropping the outermost tap of one pass at one pixel is 16 to 50 times that
(tests/test_dense_image_ops_cpu.py).  The comparison covers the tiles an image pass must compute (compare_set): elsewhere Jt is
exactly zero and the device keeps whatever an earlier pass left.  Every case also holds the contrast the call returned to the
fp64 contrast of Gy A Gx^T at RTOL.  Device figures per form: profiles/adjoint_plane_parity.txt.
"""
import functools

import numpy as np
import pytest

import adjoint_forms as af
import dense_image_ops as dio
import recon_cases as rc
import recon_grad_cases as rg
from cmax_slam_amd import _lib
from util import RTOL, rel_scalar

pytestmark = pytest.mark.gpu

R4_SIZES = [(10, 10), (64, 16), (65, 17), (128, 32), (100, 70)]  # least adjoint_ok allows; one tile; one-pixel partial tiles; a seam; ragged


def has_tables(W, H, sigma):
    """The library builds the banded G^T G tables -- and takes the composite forms (image_adjoint2<4>, image_adjoint2g, the fused tile
    pass) -- only where both sides exceed 4r (upload_gt1, cmx_context.cpp); a smaller image keeps the four-pass form whatever the
    options say.  No counter tells the forms apart (fused_evals aside), so the prints carry this rule's answer."""
    r = dio.radius(sigma)
    return r >= 1 and min(W, H) > 4 * r


def sizes_for(sigma, composite=False):
    """the sizes of a radius; for the composite forms also the least image that has tables, and one a tile wider"""
    r = dio.radius(sigma)
    sizes = list(R4_SIZES) if r == 4 else [(2 * r + 2, 2 * r + 2), (65, 2 * r + 2), (100, 70)]
    if composite:
        sizes += [s for s in [(4 * r + 1, 4 * r + 1), (65, 4 * r + 1)] if s not in sizes]
    return sizes


def check_plane(tag, jt_dev, A, sigma, measure, contrast=None, ref=None):
    """the per-pixel comparison on compare_set; returns (device error, e32), both relative to max |Jt_ref|"""
    A = np.asarray(A, np.float32)
    H, W = A.shape
    if ref is None:
        J = dio.jt_ref(A, sigma, measure)
        ref = (J,) + dio.bound(A, sigma, measure, J)
    J, b, e32, scale = ref
    mask = dio.compare_set(A, dio.radius(sigma), dio.jt_reach(sigma, measure))
    assert scale > 0 and mask.any(), tag
    assert not J[~mask].any(), tag  # (the reference vanishes outside the set: nothing is left uncompared)
    err, y, x = dio.worst_pixel(jt_dev, J, mask)
    crel = rel_scalar(contrast, dio.contrast_ref(A, sigma, measure)) if contrast is not None else 0.0
    print("adjoint_plane %s: %dx%d sigma %g measure %d  e32 %.3e  device %.3e  bound %.3e (of max |Jt| = %.6g)  contrast rel %.2e  "
          "compared %d of %d pixels" % (tag, W, H, sigma, measure, e32, err / scale, b / scale, scale, crel, int(mask.sum()), W * H))
    assert np.isfinite(jt_dev[mask]).all(), tag
    assert err <= b, ("%s: |Jt_dev - Jt_ref| = %.3e (%.3e of max |Jt|) exceeds the bound %.3e at %s; device %.9g, reference %.9g"
                      % (tag, err, err / scale, b, dio.describe_pixel(y, x, H, W), jt_dev[y, x], J[y, x]))
    if contrast is not None:
        assert crel < RTOL, (tag, contrast, crel)
    return err / scale, e32


# ------------------------------------------------------------------------------------------------------------ front end
@functools.lru_cache(maxsize=None)
def fe_case(W, H):
    p = dio.exact_packet(W, H)
    A = dio.exact_counts(p)
    A.setflags(write=False)
    return p, A


@functools.lru_cache(maxsize=None)
def fe_ref(W, H, sigma, measure):
    """(Jt_ref, bound, e32, scale) of a front-end case: computed once, shared by the forms (Jt is the same plane for measures 0 and 1)"""
    A = fe_case(W, H)[1]
    J = dio.jt_ref(A, sigma, measure)
    J.setflags(write=False)
    return (J,) + dio.bound(A, sigma, measure, J)


def fe_context(hip, W, H, sigma, measure, options=(), det=False):
    p, A = fe_case(W, H)
    fe = hip.FrontendEvaluator(p.W, p.H, p.lut)
    if det:
        fe.set_deterministic()
    for key, value in options:
        fe.set_option(getattr(_lib, "OPT_" + key), value)
    fe.set_packet(p.x, p.y, p.t_ns, p.t_ref_ns, p.fx, p.fy, p.cx, p.cy, p.batch, sigma, measure)
    return fe, A


def fe_check(tag, fe, A, sigma, measure, contrast):
    if measure != _lib.GRADIENT_MAGNITUDE:  # (the Sobel pass is one form at every size)
        tag += " [tables]" if has_tables(A.shape[1], A.shape[0], sigma) else " [no tables: four-pass]"
    out = check_plane(tag, fe.adjoint_plane(), A, sigma, measure, contrast, fe_ref(A.shape[1], A.shape[0], sigma, 2 if measure == 2 else 0))
    raw = fe.computeImageOfWarpedEvents(np.zeros(3), blur=False)
    assert np.array_equal(raw, A), "%s: the raw image is not the count per pixel" % tag
    return out


def fe_one(hip, tag, W, H, sigma, measure=0, options=(), det=False):
    fe, A = fe_context(hip, W, H, sigma, measure, options, det)
    try:
        c, g = fe.eval(np.zeros(3))
        stats = fe.stats()
        fe_check(tag, fe, A, sigma, measure, c)
        return stats
    finally:
        fe.close()


@pytest.mark.parametrize("measure", [0, 1])
@pytest.mark.parametrize("W,H", sizes_for(1.0, composite=True))
def test_fused_tile_pass(hip, W, H, measure):
    """library defaults at sigma 1: the pass rides in the splat launch wherever the image has tables"""
    stats = fe_one(hip, "defaults (fused tile pass)", W, H, 1.0, measure)
    assert stats["fused_evals"] == (1 if has_tables(W, H, 1.0) else 0) and stats["fused_redos"] == 0, stats


@pytest.mark.parametrize("W,H", sizes_for(1.0, composite=True))
def test_composite_radius_4(hip, W, H):
    stats = fe_one(hip, "FUSED_IMAGE 0 (image_adjoint2<4>)", W, H, 1.0, options=(("FUSED_IMAGE", 0),))
    assert stats["fused_evals"] == 0, stats


@pytest.mark.parametrize("W,H", sizes_for(1.0, composite=True))
def test_composite_radius_4_behind_a_cost_only_evaluation(hip, W, H):
    """f, then df at the same point: the cost-only evaluation's image pass (with the finalize in its tail) already leaves Jt --
    speculatively -- and the df reuses it"""
    fe, A = fe_context(hip, W, H, 1.0, 0, (("FUSED_IMAGE", 0),))
    try:
        c, _ = fe.eval(np.zeros(3), want_grad=False)
        s = fe.stats()
        assert s["spec_images"] == 1 and s["fused_evals"] == 0, s
        fe_check("FUSED_IMAGE 0, f (image_adjoint2<4> + tail, speculative)", fe, A, 1.0, 0, c)
    finally:
        fe.close()
    fe, A = fe_context(hip, W, H, 1.0, 0, (("FUSED_IMAGE", 0),))
    try:
        fe.eval(np.zeros(3), want_grad=False)
        c, g = fe.eval(np.zeros(3))
        s = fe.stats()
        assert s["spec_images"] == 1 and s["spec_hits"] == 1 and s["fused_evals"] == 0, s
        fe_check("FUSED_IMAGE 0, f then df (its Jt reused)", fe, A, 1.0, 0, c)
    finally:
        fe.close()


@pytest.mark.parametrize("W,H", R4_SIZES)
def test_four_pass_radius_4(hip, W, H):
    fe_one(hip, "COMPOSITE_IMAGE 0 (image_adjoint_kernel<4>)", W, H, 1.0, options=(("FUSED_IMAGE", 0), ("COMPOSITE_IMAGE", 0)))


@pytest.mark.parametrize("W,H", R4_SIZES)
def test_deterministic_planes(hip, W, H):
    stats = fe_one(hip, "deterministic", W, H, 1.0, det=True)
    assert stats["fused_evals"] == 0, stats


@pytest.mark.parametrize("sigma", [0.5, 1.7, 2.0])
def test_composite_any_radius(hip, sigma):
    for W, H in sizes_for(sigma, composite=True):
        fe_one(hip, "defaults (image_adjoint2g)", W, H, sigma)


@pytest.mark.parametrize("sigma", [0.5, 1.7, 2.0, 3.0])
def test_four_pass_any_radius(hip, sigma):
    for W, H in sizes_for(sigma):
        fe_one(hip, "COMPOSITE_IMAGE 0 (image_adjoint_kernel<-1>)", W, H, sigma, options=(("COMPOSITE_IMAGE", 0),))


@pytest.mark.parametrize("sigma", [1.0, 2.0])
def test_sobel_pass(hip, sigma):
    for W, H in sizes_for(sigma):
        fe_one(hip, "image_adjoint_sobel<%s>" % ("4" if sigma == 1.0 else "-1"), W, H, sigma, measure=_lib.GRADIENT_MAGNITUDE)


@pytest.mark.parametrize("W,H", [(10, 10), (65, 17), (100, 70)])
def test_no_blur_is_the_plane_itself(hip, W, H):
    fe, A = fe_context(hip, W, H, 0.0, 0)
    try:
        c, g = fe.eval(np.zeros(3))
        jt = fe.adjoint_plane()
        mask = dio.compare_set(A, 0, 0)
        assert mask.any() and A[mask].any()
        assert np.array_equal(jt[mask], A[mask]), "sigma 0: Jt is not A bit for bit"
        assert rel_scalar(c, dio.contrast_ref(A, 0.0, 0)) < RTOL
        assert np.array_equal(fe.computeImageOfWarpedEvents(np.zeros(3), blur=False), A)
    finally:
        fe.close()


# ------------------------------------------------------------------------------------------------------- back-end window
def be_one(hip, tag, w, IG, sigma, det=False):
    """one adjoint evaluation of a window on a fresh context -> (A, compare_set, device error, e32)"""
    be = hip.BackendEvaluator(w.W, w.H, w.lut, w.Wp, w.Hp)
    try:
        if det:
            be.set_deterministic()
        be.set_window(w.x, w.y, w.t_ns, w.order, w.knots_init, w.start_ns, w.dt_ns, w.num_fixed, w.t_next_win_beg_ns, w.batch,
                      w.sample_rate, sigma, _lib.VARIANCE, IG)
        c, g = be.eval(0.01 * np.cos(np.arange(w.P)))
        jt = be.adjoint_plane()
        old, new, alpha = be.get_plane(_lib.PLANE_IL_OLD), be.get_plane(_lib.PLANE_IL_NEW), be.alpha
    finally:
        be.close()
    A = old + new  # fp32, as the image pass composes it: IL_old + IL_new, then IG * (float) alpha + that
    if IG is not None:
        A = IG * np.float32(alpha) + A
        assert alpha > 0, alpha
    assert A.dtype == np.float32 and np.abs(g).max() > 0
    err, e32 = check_plane(tag, jt, A, sigma, 0, c)
    return A, dio.compare_set(A, dio.radius(sigma)), err, e32


def small_window():
    return rc.window("window")[0]  # 20 000 events, 256 x 128, cubic, K = 10


def test_window_sparse_scene_skips_tiles(hip):
    A, mask, _, _ = be_one(hip, "window, no map", small_window(), None, 1.0)
    assert not mask.all(), "every tile is active: the skip path did not run"


@pytest.mark.parametrize("sigma", [1.0, 1.7])
def test_window_with_a_dense_map(hip, sigma):
    """a positive map everywhere: the content reaches all four corners and every tile is active"""
    w = small_window()
    IG = np.random.default_rng(31).uniform(0.5, 2.0, (w.Hp, w.Wp)).astype(np.float32)
    A, mask, _, _ = be_one(hip, "window, dense map", w, IG, sigma)
    assert mask.all() and all(A[y, x] > 0 for y in (0, -1) for x in (0, -1))


@pytest.mark.parametrize("det,sigma", [(False, 1.0), (True, 1.0), (False, 1.7)])
def test_window_tile_list(hip, det, sigma):
    """2048 x 1056 = 2112 tiles: above the threshold at which the image passes take a compacted tile list (radius 4:
    image_adjoint2<4>'s, radius 7: image_adjoint2g's)"""
    w = af.be_window("big")
    assert -(-w.Wp // dio.TILE_X) * -(-w.Hp // dio.TILE_Y) == 2112
    A, mask, _, _ = be_one(hip, "window, tile list%s" % (", deterministic" if det else ""), w, None, sigma, det)
    assert not mask.all()


# ------------------------------------------------------------------------------------------------------ whole trajectory
def recon_make(hip, name):
    c, w = rc.CASES[name], rc.window(name)[0]
    be = hip.BackendEvaluator(rc.SENSOR[0], rc.SENSOR[1], w.lut, c["Wp"], c["Hp"])
    be.reconstruct_begin(c["order"], rg.point(name), w.start_ns, w.dt_ns, c["batch"], c["rate"])
    return be


@pytest.mark.parametrize("sigma", [0.0, 1.0, 2.0])
@pytest.mark.parametrize("name", ["pano130x96", "A"])
def test_reconstruction_contrast(hip, name, sigma):
    _, x, y, t = rc.window(name)
    be = recon_make(hip, name)
    try:
        be.reconstruct_add(x, y, t)
        A = be.reconstruct_get()
        ref = None
        for measure in (0, 1):
            c = be.reconstruct_contrast(sigma, measure, want_grad=True)
            jt = be.reconstruct_adjoint_plane()
            if sigma == 0.0:
                mask = dio.compare_set(A, 0, 0)
                assert mask.any() and np.array_equal(jt[mask], A[mask]), "sigma 0: Jt is not the plane bit for bit"
                assert rel_scalar(c, dio.contrast_ref(A, 0.0, measure)) < RTOL
                continue
            if ref is None:
                J = dio.jt_ref(A, sigma, measure)
                ref = (J,) + dio.bound(A, sigma, measure, J)
            check_plane("reconstruction %s" % name, jt, A, sigma, measure, c, ref)
    finally:
        be.close()


def test_reconstruction_bound_under_a_frozen_head(hip):
    """eval_bound after freeze_head: the votes of the frozen batches come from the base plane, Jt from the FULL plane"""
    name = "A"
    c = rc.CASES[name]
    _, x, y, t = rc.window(name)
    store = hip.EventStore(rc.SENSOR[0], rc.SENSOR[1], len(x))
    store.push(x, y, t)
    be = recon_make(hip, name)
    try:
        be.reconstruct_bind(store, 0, len(x))
        be.reconstruct_freeze_head(c["K"] // 2)
        info = be.reconstruct_frozen_info()
        assert info["frozen_batches"] > 0 and info["frozen_sampled"] < rc.sampled(len(x), c["batch"], c["rate"]), info
        con, g = be.reconstruct_eval_bound(rg.point(name), 1.0, 0)
        A, ns, ni = be.reconstruct_get(with_counts=True)
        assert ns == rc.sampled(len(x), c["batch"], c["rate"])  # the full plane: frozen and active batches
        check_plane("reconstruction A, bound, frozen head", be.reconstruct_adjoint_plane(), A, 1.0, 0, con)
    finally:
        be.close()
        store.close()


def test_reconstruction_tile_list(hip):
    """a 2048 x 1056 reconstruction: the tile-list form of the launcher on the whole-trajectory plane"""
    w = af.be_window("big")
    be = hip.BackendEvaluator(w.W, w.H, w.lut, w.Wp, w.Hp)
    try:
        be.reconstruct_begin(w.order, w.knots_init, w.start_ns, w.dt_ns, w.batch, w.sample_rate)
        be.reconstruct_add(w.x, w.y, w.t_ns)
        A = be.reconstruct_get()
        c = be.reconstruct_contrast(1.0, 0, want_grad=True)
        check_plane("reconstruction 2048x1056, tile list", be.reconstruct_adjoint_plane(), A, 1.0, 0, c)
        assert not dio.compare_set(A, 4).all()
    finally:
        be.close()


# ------------------------------------------------------------------------------------------------------------ error cases
def _status(hip, fn, *a):
    try:
        fn(*a)
    except hip.CmaxHipError as e:
        return e.status
    return _lib.OK


def test_error_cases(hip):
    L = _lib.lib()
    buf = np.zeros((128, 256), np.float32)
    ptr = buf.ctypes.data_as(_lib.c_fp)
    p, A = fe_case(100, 70)
    fe = hip.FrontendEvaluator(p.W, p.H, p.lut)
    try:
        assert _status(hip, fe.adjoint_plane) == _lib.ERR_STATE          # no packet, no evaluation
        fe.set_packet(p.x, p.y, p.t_ns, p.t_ref_ns, p.fx, p.fy, p.cx, p.cy, p.batch, 1.0, 0)
        assert _status(hip, fe.adjoint_plane) == _lib.ERR_STATE          # no evaluation yet
        assert L.cmx_diag_get_adjoint_plane(fe._ctx, _lib.DIAG_JT_RECON, ptr) == _lib.ERR_STATE  # a front end holds no reconstruction
        fe.eval(np.zeros(3))
        assert L.cmx_diag_get_adjoint_plane(fe._ctx, _lib.DIAG_JT_EVAL, None) == _lib.ERR_INVALID_ARG
        for which in (-1, 2, 99):
            assert L.cmx_diag_get_adjoint_plane(fe._ctx, which, ptr) == _lib.ERR_INVALID_ARG
        c0, g0 = fe.eval(np.zeros(3))
        a, b = fe.adjoint_plane(), fe.adjoint_plane()                    # reading changes nothing
        c1, g1 = fe.eval(np.array([0.1, 0.0, 0.0]))
        c2, g2 = fe.eval(np.zeros(3))
        assert np.array_equal(a, b) and rel_scalar(c2, c0) < 1e-12
    finally:
        fe.close()
    assert L.cmx_diag_get_adjoint_plane(None, _lib.DIAG_JT_EVAL, ptr) == _lib.ERR_INVALID_ARG
    w = small_window()
    be = hip.BackendEvaluator(w.W, w.H, w.lut, w.Wp, w.Hp)
    try:
        assert _status(hip, be.adjoint_plane) == _lib.ERR_STATE
        assert _status(hip, be.reconstruct_adjoint_plane) == _lib.ERR_STATE   # no reconstruction
        be.reconstruct_begin(w.order, w.knots_init, w.start_ns, w.dt_ns, w.batch, w.sample_rate)
        be.reconstruct_add(w.x, w.y, w.t_ns)
        be.reconstruct_contrast(1.0, 0, want_grad=False)
        assert _status(hip, be.reconstruct_adjoint_plane) == _lib.ERR_STATE   # a cost-only image pass makes no Jt
        be.reconstruct_contrast(1.0, 0, want_grad=True)
        assert be.reconstruct_adjoint_plane().any()
        assert _status(hip, be.adjoint_plane) == _lib.ERR_STATE               # the window's plane is another one
        assert L.cmx_diag_get_adjoint_plane(be._ctx, _lib.DIAG_JT_RECON, None) == _lib.ERR_INVALID_ARG
    finally:
        be.close()
    grp = hip.BackendEvaluator(w.W, w.H, w.lut, w.Wp, w.Hp, devices=[0, 0])
    try:
        for which in (_lib.DIAG_JT_EVAL, _lib.DIAG_JT_RECON):
            assert L.cmx_diag_get_adjoint_plane(grp._ctx, which, ptr) == _lib.ERR_INVALID_ARG
    finally:
        grp.close()
