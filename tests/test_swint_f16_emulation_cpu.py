"""tools/swint_f16_emulation.py (the CPU study behind the fp16 Swin path's storage plan) is itself pinned: with nothing rounded it is
``tests.swin_ref.model_forward`` within 1e-5 (the bar of tests/test_swint_cpu.py; measured 1.6e-6 or less -- the emulation scales the
q k^T product where the reference scales q, and writes the softmax out), and its ``f16`` mode stays inside the fp16 bar (5e-3 of
max(1, scale)) on every configuration of its table, while differing from the reference by more than 1e-5: the rounding is on."""
import functools
import importlib.util
import os

import pytest

from tests import swin_ref as R

_spec = importlib.util.spec_from_file_location("swint_f16_emulation", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "swint_f16_emulation.py"))
E = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(E)

CASES = E.cases()


@functools.lru_cache(maxsize=None)
def _reference(i):
    """State dict, reference heads and reference block activations of case i: computed once, shared, never modified."""
    _label, bb, heads, mt, img, seed = CASES[i]
    sd = R.init_state_swint(bb, heads, mt, seed=seed)
    collect = {}
    ref = R.model_forward(sd, bb, heads, mt, img, collect=collect)
    return sd, ref, collect


def test_cases_are_the_table():
    labels = [c[0] for c in CASES]
    assert len(labels) == 7, labels  # six table rows; the Swin-tiny row holds two sizes
    assert labels[0].startswith("SMALL w7 2x64x96") and labels[1].startswith("SMALL w7 2x64x192")
    assert labels[2].startswith("SMALL w4") and labels[3].startswith("SMALL w8")
    assert tuple(CASES[4][4].shape) == (1, 3, 64, 64) and tuple(CASES[5][4].shape) == (1, 3, 96, 96) and CASES[5][1]["model_type"] == "tiny"
    assert CASES[6][1]["model_type"] == "small" and R.arch_of(CASES[6][1])["depths"][2] == 18


@pytest.mark.parametrize("i", [0, 1, 2, 3, 4])
def test_fp32_mode_is_the_reference(i):
    """Heads and every labelled activation, on the shifted / padded / mixed-shift / window 4 and 8 / Swin-tiny configurations."""
    _label, bb, heads, mt, img, _seed = CASES[i]
    sd, ref, collect_ref = _reference(i)
    collect = {}
    got = E.forward(sd, bb, heads, mt, img, "fp32", collect=collect)
    assert set(got) == set(ref)
    for k, t in ref.items():
        assert (got[k] - t).abs().max().item() <= 1e-5 * max(1.0, t.abs().max().item()), k
    assert set(collect) == set(collect_ref)
    for k, t in collect_ref.items():
        assert (collect[k] - t).abs().max().item() <= 1e-5 * max(1.0, t.abs().max().item()), k


@pytest.mark.parametrize("i", range(len(CASES)))
def test_f16_mode_rounds_and_stays_inside_the_bar(i):
    label, bb, heads, mt, img, _seed = CASES[i]
    sd, ref, _ = _reference(i)
    err = E.head_error(E.forward(sd, bb, heads, mt, img, "f16"), ref)
    print(label, f"{err:.2e}")
    assert 1e-5 < err <= 5e-3, (label, err)


def test_f16_res32_mode_rounds_and_stays_inside_the_bar():
    """Form (b) (fp32 residual stream) on the first configuration: a different result from form (a), inside the bar too."""
    _label, bb, heads, mt, img, _seed = CASES[0]
    sd, ref, _ = _reference(0)
    a = E.forward(sd, bb, heads, mt, img, "f16")
    b = E.forward(sd, bb, heads, mt, img, "f16_res32")
    assert any(not (a[k] == b[k]).all() for k in a)
    assert 1e-5 < E.head_error(b, ref) <= 5e-3
