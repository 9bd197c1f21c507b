"""No GPU: what tests/test_gpu_call_sequences.py takes for granted about tests/seq_cases.py -- the far points really are far (votes
in tiles no chunk of the sort reaches) and really cause no new sort (3 % of the events or fewer leave their windows), the
generator gives the same list for the same seed, the seeds that run cover the whole alphabet, and no evaluation point has a
gradient so small that 1e-5 of it would be the arithmetic's own noise."""
import numpy as np
import pytest

import seq_cases as sc


@pytest.fixture(scope="module", autouse=True)
def _oracle(oracle):
    return oracle


def _same(a, b):
    if isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
        return np.array_equal(a, b)
    return a == b


# the points at which the directed tests sort: OMEGA0 for every packet (their first evaluation)
@pytest.mark.parametrize("name", sc.SPARSE)
def test_far_point_conditions(name):
    p = sc.packet(name)
    assert len(p.x) <= 30_000 and (p.W, p.H) == (240, 180) and np.all(np.diff(p.t_ns) >= 0)
    om = sc.far_point(name, sc.OMEGA0)
    # (a) no new sort: 3 % of the events or fewer move by more than the window margin ...
    assert sc.moved_share(p, sc.OMEGA0, om) <= sc.REBIN_FRAC
    # ... and the share the library itself will count (votes outside their windows) lies in (0, 3 %]
    assert 0 < sc.fallback_share(p, sc.OMEGA0, om) <= sc.REBIN_FRAC
    assert sc.fallback_share(p, sc.OMEGA0, om, sc.FUSE_REACH) > 0     # ... some of them beyond the reach (kFuseUnsafe)
    # (b) votes in a tile more than kFuseNbr tiles from every tile occupied at the sort
    far = sc.unreached_tiles(name, sc.OMEGA0, om)
    assert far
    ref = sc.fe_oracle(name)
    occ = np.argwhere(sc.tiles_of(ref.iwe(sc.OMEGA0, blur=False)))
    for r, c in far:
        assert np.all(np.maximum(np.abs(occ[:, 0] - r), np.abs(occ[:, 1] - c)) > sc.FUSE_NBR)
    # the near steps of the directed tests stay inside every window, and the packet is sparse: most tiles are empty
    for k in (1, 2, 3):
        assert sc.fallback_share(p, sc.OMEGA0, sc.OMEGA0 + k * sc.EPS) == 0
    assert len(occ) <= 10 < 8 * 6
    # what a missed clear leaves behind: half a percent of the votes or more, in a blob (1e-4 of the contrast, ten times the bar)
    iwe = ref.iwe(om, blur=False)
    left = sum(iwe[r * 32:(r + 1) * 32, c * 32:(c + 1) * 32].sum() for r, c in far)
    assert 0.004 * len(p.x) < left < 0.03 * len(p.x)


def test_mirrored_packet_reaches_the_border_and_the_ragged_tile_row():
    occ = np.argwhere(sc.tiles_of(sc.fe_oracle("B").iwe(sc.OMEGA0, blur=False)))
    assert occ[:, 0].max() == 5 and occ[:, 1].max() == 7     # last tile row (20 px high) and last tile column (16 px wide)


def test_two_group_packet_has_a_step_within_reach_and_one_beyond():
    p = sc.packet("C")
    near = sc.reach_point("C", sc.OMEGA0)
    assert 0 < sc.fallback_share(p, sc.OMEGA0, near) <= sc.REBIN_FRAC     # leaves windows ...
    assert not sc.unreached_tiles("C", sc.OMEGA0, near)                   # ... but no tile beyond the reach
    assert sc.fallback_share(p, sc.OMEGA0, near, sc.FUSE_REACH) == 0
    far = sc.far_point("C", sc.OMEGA0)
    assert sc.unreached_tiles("C", sc.OMEGA0, far) and sc.fallback_share(p, sc.OMEGA0, far, sc.FUSE_REACH) > 0


@pytest.mark.parametrize("name", sc.SPARSE)
def test_resort_point_leaves_the_windows(name):
    om = sc.resort_point(name, sc.OMEGA0)
    assert sc.fallback_share(sc.packet(name), sc.OMEGA0, om) > sc.REBIN_FRAC


def test_dense_packet_is_dense():
    assert sc.tiles_of(sc.fe_oracle("D").iwe(sc.OMEGA0, blur=False)).all()


@pytest.mark.parametrize("seed", sc.FE_SEEDS)
def test_frontend_generator_is_reproducible_and_keeps_the_gradient_rule(seed):
    ops = sc.fe_walk(seed)
    again = sc.fe_walk.__wrapped__(seed)   # (past the cache)
    assert 30 <= len(ops) <= 40 and len(ops) == len(again)
    for a, b in zip(ops, again):
        assert a.keys() == b.keys() and all(_same(a[k], b[k]) for k in a), (seed, a, b)
    # the rule, recomputed from the oracle over the list as it stands
    grads = []
    for o in ops:
        ref = sc.fe_oracle(o["packet"])
        if o["op"] in ("eval", "eval_f", "hint_df"):
            c, g = ref.eval(o["x"])
            assert c == o["c"] and np.array_equal(g, o["g"])
            grads.append(np.abs(g).max())
        elif o["op"] in ("eval_many", "eval_each"):
            assert 1 <= len(o["xs"]) <= 4
            for x, c0, g0 in zip(o["xs"], o["cs"], o["gs"]):
                c, g = ref.eval(x)
                assert c == c0 and np.array_equal(g, g0)
                grads.append(np.abs(g).max())
        if o.get("kind") == "same":
            assert np.array_equal(o["x"], ops[o["same_as"]]["x"]) and ops[o["same_as"]] is ops[ops.index(o) - 1]
    assert min(grads) >= sc.GRAD_FLOOR * max(grads), (seed, min(grads), max(grads))


def test_frontend_seeds_cover_the_alphabet():
    seen = set()
    for seed in sc.FE_SEEDS:
        seen |= sc.fe_alphabet(sc.fe_walk(seed))
    assert seen >= sc.FE_ALPHABET, sorted(sc.FE_ALPHABET - seen)
    assert {o["packet"] for seed in sc.FE_SEEDS for o in sc.fe_walk(seed)} == set(sc.PACKETS)
    for seed in sc.FE_DET_SEEDS:
        det = sc.fe_walk(seed, True)
        assert 30 <= len(det) <= 40 and not any(o.get("deriv") for o in det)


@pytest.mark.parametrize("seed", sc.BE_SEEDS)
def test_backend_generator_is_reproducible_and_keeps_the_gradient_rule(seed):
    ops = sc.be_walk(seed)
    again = sc.be_walk.__wrapped__(seed)   # (past the cache)
    assert 30 <= len(ops) <= 40 and len(ops) == len(again)
    for a, b in zip(ops, again):
        assert a.keys() == b.keys() and all(_same(a[k], b[k]) for k in a), (seed, a, b)
    grads = [np.abs(o["g"]).max() for o in ops if "g" in o] + [np.abs(g).max() for o in ops if "gs" in o for g in o["gs"]]
    assert min(grads) >= sc.GRAD_FLOOR * max(grads), (seed, min(grads), max(grads))
    for i, o in enumerate(ops):   # the blend factor belongs to the first evaluation after a set_window: one always follows
        if o["op"] == "set_window":
            assert ops[i + 1]["op"] == "eval"


def test_backend_seeds_cover_the_alphabet_and_the_windows_are_sparse():
    seen = set()
    for seed in sc.BE_SEEDS:
        seen |= sc.be_alphabet(sc.be_walk(seed))
    assert seen >= sc.BE_ALPHABET, sorted(sc.BE_ALPHABET - seen)
    for seed in sc.BE_DET_SEEDS:
        assert all(o["fast"] for o in sc.be_walk(seed, True) if o["op"] == "path")
    for which in (0, 1):
        w = sc.be_window(which)
        assert w.Wp * w.Hp <= 512 * 256 and len(w.x) <= 40_000
        ref = sc.be_oracle(which)
        sc.be_oracle_set_window(ref, which, "none")
        ref.eval(np.zeros(w.P))
        occ = sc.tiles_of(ref.IL_old + ref.IL_new)
        assert 0 < occ.mean() < 0.5    # the camera sees a part of the panorama: most tiles hold no vote
        big = np.tile([0.0, 0.25, 0.0], w.P // 3)
        ref.eval(big)
        assert (sc.tiles_of(ref.IL_old + ref.IL_new) & ~occ).any()   # the big step votes into tiles that were empty
