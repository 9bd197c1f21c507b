"""CPU: the inputs of the whole-trajectory reconstruction tests (tests/test_gpu_recon.py) are not empty comparisons, and the rule
those tests rely on -- vote loops over slices cut at batch multiples add up to the loop over the whole stream -- holds in the
oracle itself.  Needs no GPU and nothing of the reconstruction."""
import numpy as np
import pytest

import recon_cases as rc
from util import RTOL, rel_img


@pytest.mark.parametrize("name", sorted(rc.CASES))
def test_oracle_plane_holds_at_least_half_the_sampled_events(oracle, name):
    c = rc.CASES[name]
    plane = rc.oracle_plane(oracle, name)
    n_sampled = rc.sampled(c["N"], c["batch"], c["rate"])
    votes = float(plane.sum(dtype=np.float64))
    assert plane.shape == (c["Hp"], c["Wp"])
    assert votes >= 0.5 * n_sampled, (votes, n_sampled)
    assert votes <= n_sampled * (1 + 1e-6)
    if c["N"] >= 65:
        assert n_sampled > 0 and votes > 0


def test_sampling_counts_of_the_two_main_configurations():
    assert rc.sampled(60_007, 100, 1) == 60_007
    assert rc.sampled(30_001, 64, 3) == 10_313
    assert rc.sampled(65, 64, 1) == 64 and rc.sampled(2, 64, 1) == 2 and rc.sampled(1, 64, 1) == 0


def test_border_rule_drops_votes_in_the_poles_configuration(oracle):
    c = rc.CASES["poles"]
    votes = float(rc.oracle_plane(oracle, "poles").sum(dtype=np.float64))
    assert votes < rc.sampled(c["N"], c["batch"], c["rate"]) - 1


@pytest.mark.parametrize("name,at", [("A", (70 * 100, 400 * 100)), ("B", (7 * 64, 100 * 64))])
def test_oracle_over_slices_at_batch_multiples_equals_the_whole(oracle, name, at):
    _, x, y, t = rc.window(name)
    total = np.zeros_like(rc.oracle_plane(oracle, name), dtype=np.float64)
    for lo, hi in rc.cuts(name, *at):
        total += rc.oracle_loop(oracle, name, x[lo:hi], y[lo:hi], t[lo:hi])
    r = rel_img(total, rc.oracle_plane(oracle, name))
    print("%s: sliced vs whole %.2e" % (name, r))
    assert r < RTOL
