"""CPU: the probe packets of the per-event front-end vote tests (tests/fe_probe_cases.py), from the reference side alone.

1. At every omega of a case's list every pixel holds at most one event's vote and every voting cell has a ring of one empty pixel
   around it; no u, v of a non-zero omega lies within INT_MARGIN of an integer; the cells are gather_ref.fe_events' own.
2. Coverage (every case but tiny, far and sparse): at omega = 0, where the pixel chooses the cell, at least 5 voting events on
   each of the last accepted columns and rows (xx = 1, W - 3, yy = 1, H - 3) and at least 5 events that do not vote but lie within kBinMargin
   of the accepted region (the sensor's outermost pixels: a sensor pixel cannot lie further out at omega = 0); at W3 at least 5
   events beyond kBinMargin (the sort's no-window sentinel); every sort tile holds a voting event; two_slices makes three slices.
3. Between W1 and W2 no event moves 8 px, between W1 and W3 some move more than 16.
4. The host model of the sort: no vote leaves its window when the sort was made at the evaluation's own omega, nor from W1 to W2;
   from W1 to W3 some do -- in every case but tiny (33 x 35 is smaller than one window: the model's count there is 0).
5. Five mutations of the reference's own arithmetic -- every event warped with the next batch's dt (and the last event of one
   batch alone), one event with another event's bearing from the same sort tile, the last accepted column rejected, one event's
   four weights permuted, one vote of the previous omega left in the plane -- each exceed BOUND at least CATCH = 100 times at some
   pixel, and fail compare(), the function the GPU test calls on a device plane.  The unmutated reference and the host's fp32 votes
   (gather_ref.forward_plane) pass it."""
import numpy as np
import pytest

import fe_probe_cases as fp
import gather_ref as gr


@pytest.mark.parametrize("name", list(fp.CASES))
def test_cells_are_disjoint_with_an_empty_ring_at_every_omega(name):
    c, p = fp.CASES[name], fp.packet(name)
    assert len(p.x) == c.n and -(-c.n // c.batch) >= 2 and c.n % c.batch != 0          # a ragged last batch
    dts = fp.batch_dts(p.t_ns, p.t_ref_ns, p.batch)
    assert np.abs(dts).min() > 1e-5                                                    # no batch sits on the reference time
    for om in c.omegas:
        ev = fp.events(name, om)
        xx, yy, ok, u, v = fp._all_cells(name, om)
        assert np.array_equal(ev.xx, xx[ok]) and np.array_equal(ev.yy, yy[ok]) and np.array_equal(ev.src, np.flatnonzero(ok))
        cnt = np.zeros((p.H, p.W), np.int64)
        for oy in (0, 1):
            for ox in (0, 1):
                np.add.at(cnt, (ev.yy + oy, ev.xx + ox), 1)
        assert cnt.max() <= 1, (name, om)
        block = sum(cnt[ev.yy + oy, ev.xx + ox] for oy in (-1, 0, 1, 2) for ox in (-1, 0, 1, 2))
        assert (block == 4).all(), (name, om, int((block != 4).sum()))                # the cell's own four pixels and nothing else
        ref, mask = fp.reference(name, om)
        assert mask.sum() == 4 * ev.n and not ref[~mask].any()
        if any(om):
            fin = np.isfinite(u) & np.isfinite(v)
            margin = min(np.abs(u[fin] - np.rint(u[fin])).min(), np.abs(v[fin] - np.rint(v[fin])).min())
            assert margin >= fp.INT_MARGIN, (name, om, margin)
        elif not c.unit_lut:
            assert np.array_equal(u, p.x.astype(np.float64)) and np.array_equal(v, p.y.astype(np.float64))
        print("probe %s omega %s: %d events, %d vote" % (name, om, c.n, ev.n))
        assert ev.n >= (10 if name == "tiny" else 100)


def test_far_case_leaves_the_image():
    p = fp.packet("far")
    xx, yy, ok, u, v = fp._all_cells("far", fp.FAR_OMEGA)
    x, y = p.x.astype(np.int64), p.y.astype(np.int64)
    dt = fp.batch_dts(p.t_ns, p.t_ref_ns, p.batch)[np.arange(len(x)) // p.batch]
    b = p.lut.reshape(-1, 3)[y * p.W + x]
    rz = b[:, 2] + ((fp.FAR_OMEGA[0] * dt) * b[:, 1] - (fp.FAR_OMEGA[1] * dt) * b[:, 0])
    print("far: %d of %d events vote, rz from %.3f to %.3f, %d with rz < 0, |rz| min %.2e" % (ok.sum(), len(x), rz.min(), rz.max(),
                                                                                           (rz < 0).sum(), np.abs(rz).min()))
    assert ok.sum() < len(x) // 4 and (rz < 0).sum() >= 5 and np.abs(rz).min() < 0.01
    assert fp.predicted_fallback("far", fp.FAR_OMEGA, fp.FAR_OMEGA) == 0


@pytest.mark.parametrize("name", fp.COVERAGE_CASES)
def test_coverage_of_the_accept_rule_and_the_sort(name):
    p = fp.packet(name)
    W, H = p.W, p.H
    ev = fp.events(name, fp.W0)
    lines = [int((ev.xx == 1).sum()), int((ev.xx == W - 3).sum()), int((ev.yy == 1).sum()), int((ev.yy == H - 3).sum())]
    tx, ty, has_win = fp.sort_keys(name, fp.W0)
    _, _, ok, _, _ = fp._all_cells(name, fp.W0)
    near = int((~ok & has_win).sum())
    _, _, has_win3 = fp.sort_keys(name, fp.W3)
    beyond = int((~has_win3).sum())
    tiles = len(set(zip(tx[ok].tolist(), ty[ok].tolist())))
    print("probe %s: voting events on xx = 1, W - 3, yy = 1, H - 3 at omega 0: %s; not accepted within the margin %d; beyond it at W3 %d; "
          "%d sort tiles hold votes; %d sort slices" % (name, lines, near, beyond, tiles, fp.sort_slices(len(p.x))))
    assert min(lines) >= 5 and near >= 5 and beyond >= 5
    assert tiles == -(-(W - 3) // fp.TILE) * -(-(H - 3) // fp.TILE)
    if name == "two_slices":
        assert len(p.x) > 2 * 4096 and fp.sort_slices(len(p.x)) >= 3


@pytest.mark.parametrize("name", [k for k in fp.CASES if k != "far"])
def test_drift_and_the_sort_model(name):
    d12, d13 = fp.displacement(name, fp.W1, fp.W2), fp.displacement(name, fp.W1, fp.W3)
    assert d12.max() < 8.0 and d13.max() > 16.0, (d12.max(), d13.max())
    for om in fp.OMEGAS:
        assert fp.predicted_fallback(name, om, om) == 0 and not fp.predicted_unsafe(name, om, om)
    assert fp.predicted_fallback(name, fp.W1, fp.W2) == 0
    n13 = fp.predicted_fallback(name, fp.W1, fp.W3)
    print("probe %s: W1 -> W2 moves at most %.2f px, W1 -> W3 up to %.1f px; %d of %d votes leave their windows, beyond the reach: %s"
          % (name, d12.max(), d13.max(), n13, fp.events(name, fp.W3).n, fp.predicted_unsafe(name, fp.W1, fp.W3)))
    if name == "tiny":   # 33 x 35 is smaller than one 64 x 64 window
        assert n13 == 0
    else:
        assert n13 > 0


def test_sparse_case_leaves_most_sort_tiles_empty():
    p = fp.packet("sparse")
    total = -(-p.W // fp.TILE) * -(-p.H // fp.TILE)
    used = []
    for om in fp.OMEGAS:
        tx, ty, _ = fp.sort_keys("sparse", om)
        _, _, ok, _, _ = fp._all_cells("sparse", om)
        used.append(set(zip(tx[ok].tolist(), ty[ok].tolist())))
    print("probe sparse: sort tiles with votes %s of %d; W3 reaches %d tiles W1 does not" % ([len(u) for u in used], total,
                                                                                          len(used[3] - used[1])))
    assert all(len(u) <= total // 3 for u in used) and len(used[3] - used[1]) >= 2


def test_both_outcomes_of_the_jump_are_among_the_cases():
    """W1 -> W3 stays within the fused tiles' reach in one case (the count is read) and leaves it in another (the evaluation is
    repeated behind a fresh sort)"""
    unsafe = {name: fp.predicted_unsafe(name, fp.W1, fp.W3) for name in fp.COVERAGE_CASES}
    assert any(unsafe.values()) and not all(unsafe.values()), unsafe


@pytest.mark.parametrize("name,omega,prev", [("qvga", fp.W1, fp.W0), ("qvga", fp.W3, fp.W2), ("qvga_b257", fp.W2, fp.W1),
                                             ("one_tile_row", fp.W1, fp.W0), ("two_slices", fp.W1, fp.W0), ("unit_lut", fp.W1, fp.W0)])
def test_mutations_exceed_the_bound(name, omega, prev):
    ev = fp.events(name, omega)
    ref, _ = fp.reference(name, omega)
    assert fp.compare("reference", ref, name, omega) == 0.0
    host32 = fp.compare("host fp32 votes", gr.forward_plane(ev), name, omega)   # the kernels' weight arithmetic, on the host
    assert host32 <= 3.0 / 4.0                                                   # (2.5 * 2^-24 at most, and a rounding to spare)
    figures = []
    for kind, plane in fp.mutated_planes(name, omega, prev).items():
        ratio = float(np.abs(plane - ref).max()) / fp.BOUND
        figures.append("%s %.3g" % (kind, ratio))
        assert ratio >= fp.CATCH, (name, kind, ratio)
        with pytest.raises(AssertionError):
            fp.compare(kind, plane, name, omega)
        with pytest.raises(AssertionError):
            fp.compare(kind, plane.astype(np.float32), name, omega)
    print("probe %s omega %s: host fp32 votes %.3f bounds; mutations, worst pixel over bound: %s"
          % (name, omega, host32, ", ".join(figures)))
