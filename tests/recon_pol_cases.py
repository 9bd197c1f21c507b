"""The polarity of every recon_cases configuration and the numpy reference of the signed-panorama tests
(tests/test_gpu_recon_pol.py): the per-event reference of tests/recon_warp_cases.py, its events with flags == 3 split by
polarity, each half voted again with the oracle's own vote functions.  tests/test_recon_pol_cpu.py checks on the CPU that the
two halves add up to the oracle's plane and that neither is empty before anything is compared with them."""
import numpy as np

import recon_cases as rc
import recon_warp_cases as wc

# the configurations the GPU tests vote (the edge counts n0 / n1 / n2 hold too few events for two non-empty halves)
DEFAULT_MODE = ("A", "B", "batch3", "batch5000", "poles", "pano130x96")
USED = tuple(dict.fromkeys(wc.CLOSURE + DEFAULT_MODE + ("window",)))
EDGE = wc.EDGE

_pol, _refs = {}, {}


def polarity(name):
    """one byte per event of the configuration, 0 (OFF) or 1 (ON): default_rng(1000 + seed).integers(0, 2, N); read-only"""
    if name not in _pol:
        c = rc.CASES[name]
        p = np.random.default_rng(1000 + c["seed"]).integers(0, 2, c["N"]).astype(np.uint8)
        p.setflags(write=False)
        _pol[name] = p
    return _pol[name]


def split(fl, pol):
    """(flags of the ON events, flags of the OFF events): the other half's flags are cleared, so revote leaves it out"""
    on = np.asarray(pol) != 0
    return np.where(on, fl, 0).astype(np.uint8), np.where(on, 0, fl).astype(np.uint8)


def reference_of(px, py, fl, pol, Hp, Wp):
    """(ON plane, OFF plane, n_on, n_off) of one polarity vote loop over events whose coordinates and flags are known"""
    fl_on, fl_off = split(fl, pol)
    return (wc.revote(px, py, fl_on, Hp, Wp), wc.revote(px, py, fl_off, Hp, Wp),
            int(np.count_nonzero(fl_on == 3)), int(np.count_nonzero(fl_off == 3)))


def reference(po, name):
    """the reference on the configuration's whole stream at its true knots (computed once, read-only)"""
    if name not in _refs:
        c = rc.CASES[name]
        px, py, fl = wc.reference(po, name)
        out = reference_of(px, py, fl, polarity(name), c["Hp"], c["Wp"])
        for a in out[:2]:
            a.setflags(write=False)
        _refs[name] = out
    return _refs[name]
