"""No GPU: the properties tests/test_gpu_adjoint_forms.py relies on in tests/adjoint_forms.py."""
import numpy as np

import adjoint_forms as af


def test_every_form_has_a_known_script_and_kind():
    scripts = {"f_df", "f_df_same", "hint", "many", "split", "three", "solve"}
    for name, (kinds, script, setup) in af.FORMS.items():
        assert kinds in ("f", "b", "fb") and script in scripts, name
        assert set(setup) <= {"scale", "comm", "det", "options", "scene", "measure"}, name
    assert set(af.forms("f")) | set(af.forms("b")) == set(af.FORMS)
    assert af.DETERMINISTIC == ("deterministic", "big_deterministic")


def test_no_comparison_is_empty_but_the_empty_scene():
    for kind in "fb":
        for name in af.forms(kind):
            if af.FORMS[name][1] == "solve":
                continue
            (c0, g0), (c1, g1) = af.expected(kind, name, 0), af.expected(kind, name, 1)
            if af.FORMS[name][2].get("scene") == "empty":
                assert c0 == 0 and c1 == 0 and not g0.any() and not g1.any(), (kind, name)
                continue
            assert c0 > 0 and c1 > 0 and abs(c0 - c1) > 1e-4 * c0, (kind, name, c0, c1)   # two points the tolerance tells apart
            assert min(np.abs(g0).max(), np.abs(g1).max()) > 1e-3 * c0, (kind, name)


def test_the_hint_opens_and_shuts_the_gate():
    """mode 1 opens the gate when f = -contrast < threshold = -contrast * scale, contrast > 0: scale 0.5 opens, 2 does not"""
    for kind in "fb":
        c = af.expected(kind, "hint_open", 0)[0]
        assert -c < -c * af.FORMS["hint_open"][2]["scale"] and not -c < -c * af.FORMS["hint_shut"][2]["scale"]


def test_the_big_panorama_is_just_above_the_tile_list_threshold():
    w = af.be_window("big")
    tiles = -(-w.Wp // 64) * -(-w.Hp // 16)   # kAdjTX x kAdjTY
    assert 2048 < tiles <= 2048 + 64, tiles     # kTileListMin
    assert af.be_window("small").P == w.P
