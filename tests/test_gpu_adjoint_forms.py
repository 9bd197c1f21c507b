"""-m gpu: every form of an adjoint evaluation once (tests/adjoint_forms.py), held to the oracle AND to what it launches.

The header comments of cmx_pipeline.cpp and cmx_chain.cpp promise launch counts ("two launches instead of three", "no per-batch
kernel, no reduce_gpartials launch", a df at the point of a cost-only evaluation starts at the gather).  Here they are asserted:
per form, the launches per class that timing_get counts (image, gather, final, batch) and the stats() deltas of the speculative
image, the gated pass, image reuse and the host finalize.  The integers are what the library reported on an MI355X before the
evaluation's host code was rearranged into named steps (profiles/adjoint_refactor.txt); nothing in them is a tolerance.
"""
import pytest

import adjoint_forms as af
from util import RTOL, rel_scalar, rel_vec

pytestmark = pytest.mark.gpu

# (image, gather, final, batch) launches, then (spec_images, spec_hits, gated_launches, gated_hits, reuse_hits, host_finalize_evals)
EXPECTED = {
    ("f", "f_df_new"): ((1, 1, 0, 0), (1, 0, 0, 0, 0, 1)),     # (the df's image pass rides in its splat launch: no image-class launch)
    ("f", "f_df_same"): ((1, 1, 0, 0), (1, 1, 0, 0, 1, 1)),    # the df starts at the gather
    ("f", "hint_open"): ((1, 0, 0, 0), (1, 1, 1, 1, 1, 0)),    # the gated gather is not a sample of the gather class; the df launches nothing
    ("f", "hint_shut"): ((1, 1, 0, 0), (1, 1, 1, 0, 1, 1)),
    ("f", "eval_many"): ((2, 2, 0, 0), (0, 0, 0, 0, 0, 0)),
    ("f", "split_2p"): ((1, 1, 1, 0), (0, 0, 0, 0, 0, 0)),
    ("f", "split_rows"): ((3, 2, 2, 0), (0, 0, 0, 0, 1, 0)),
    ("f", "deterministic"): ((2, 2, 0, 0), (1, 1, 0, 0, 1, 0)),
    ("f", "tail_0"): ((1, 2, 3, 0), (1, 1, 0, 0, 1, 0)),
    ("f", "tail_1"): ((1, 2, 0, 0), (1, 1, 0, 0, 1, 0)),
    ("f", "tail_2"): ((1, 2, 0, 0), (1, 1, 0, 0, 1, 0)),
    ("f", "tail_4"): ((1, 2, 0, 0), (1, 1, 0, 0, 1, 2)),
    ("f", "empty"): ((3, 0, 2, 0), (0, 0, 0, 0, 1, 0)),
    ("f", "gradmag"): ((2, 2, 1, 0), (1, 1, 0, 0, 1, 2)),
    ("b", "f_df_new"): ((2, 1, 0, 0), (1, 0, 0, 0, 0, 0)),
    ("b", "f_df_same"): ((1, 1, 0, 0), (1, 1, 0, 0, 1, 0)),
    ("b", "hint_open"): ((1, 0, 0, 0), (1, 1, 1, 1, 1, 0)),
    ("b", "hint_shut"): ((1, 1, 0, 0), (1, 1, 1, 0, 1, 0)),
    ("b", "eval_many"): ((2, 2, 0, 0), (0, 0, 0, 0, 0, 0)),
    ("b", "split_2p"): ((1, 1, 1, 1), (0, 0, 0, 0, 0, 0)),
    ("b", "split_rows"): ((3, 2, 2, 0), (0, 0, 0, 0, 1, 0)),   # no per-batch kernel
    ("b", "deterministic"): ((2, 2, 2, 2), (1, 1, 0, 0, 1, 0)),
    ("b", "tail_0"): ((2, 2, 3, 2), (1, 1, 0, 0, 1, 0)),
    ("b", "tail_1"): ((2, 2, 0, 0), (1, 1, 0, 0, 1, 0)),       # one kernel: gather, per-batch pass and finalize
    ("b", "tail_2"): ((2, 2, 0, 2), (1, 1, 0, 0, 1, 0)),
    ("b", "tail_4"): ((2, 2, 0, 0), (1, 1, 0, 0, 1, 0)),
    ("b", "empty"): ((3, 0, 2, 0), (0, 0, 0, 0, 1, 0)),
    ("b", "fold_0"): ((2, 2, 0, 2), (1, 1, 0, 0, 1, 0)),
    ("b", "big"): ((2, 2, 0, 0), (1, 1, 0, 0, 1, 0)),
    ("b", "big_deterministic"): ((2, 2, 3, 2), (1, 1, 0, 0, 1, 0)),
}
# the solve forms: (chain_solves, chain_takeovers, chain_warm_starts).  The number of slots follows the line search, which follows
# the last bits of sums made with fp32 atomics: it is reported (tools/adjoint_forms_walk.py), not asserted
EXPECTED_CHAIN = {
    "solve_default": (1, 0, 0),
    "solve_4": (1, 0, 0),
}

TIMED = [(k, n) for k in "fb" for n in af.forms(k) if af.FORMS[n][1] != "solve"]
SOLVES = [n for n in af.forms("f") if af.FORMS[n][1] == "solve"]


def _check_results(kind, name, results):
    assert results, (kind, name)
    for i, c, g in results:
        c_ref, g_ref = af.expected(kind, name, i)
        print("%s %s x%d: contrast %.9g (oracle %.9g, rel %.2e)%s" % (kind, name, i, c, c_ref, rel_scalar(c, c_ref),
                                                                      " gradient rel %.2e" % rel_vec(g, g_ref) if g is not None else ""))
        assert rel_scalar(c, c_ref) < RTOL, (kind, name, i, c, c_ref)
        if g is not None:
            assert rel_vec(g, g_ref) < RTOL, (kind, name, i, g, g_ref)


@pytest.mark.parametrize("kind,name", TIMED)
def test_form_results_launches_and_counters(hip, oracle, kind, name):
    rec = af.run_form(hip, kind, name)
    _check_results(kind, name, rec["results"])
    launches = tuple(rec["launches"][k] for k in af.CLASSES)
    stats = tuple(rec["stats"][k] for k in af.STATS)
    print(kind, name, "launches", dict(zip(af.CLASSES, launches)), "stats", dict(zip(af.STATS, stats)))
    assert (launches, stats) == EXPECTED[(kind, name)], (kind, name)


@pytest.mark.parametrize("name", SOLVES)
def test_solve_forms(hip, oracle, name):
    """The device-driven solve queues the cost-only and gated forms as slots (CMX_OPT_CHAIN_SOLVE 4) or its own self-gating slots
    (default).  final_cost is the machine's f at the returned x (tests/test_gpu_call_sequences.py): its negative is the oracle's
    contrast there."""
    rec = af.run_form(hip, "f", name)
    print(name, rec)
    c_ref = af._fe_oracle("small", af.po.VARIANCE).eval(rec["x"], False)[0]
    assert rel_scalar(-rec["final_cost"], c_ref) < RTOL, (name, rec, c_ref)
    assert rec["stats"]["chain_slots"] >= 2, rec
    assert tuple(rec["stats"][k] for k in af.CHAIN_STATS) == EXPECTED_CHAIN[name], (name, rec)
