"""The host side of the backward route record, and the references of tests/_backward_cases.py on their own: the float64 yardstick of
tests/test_gpu_backward_routes.py is only as sharp as torch's fp32 step is close to it."""
import itertools
import re
import time

import pytest

from sleap_nn_amd import _lib as L
from tests import _backward_cases as T

E_REF_CAP = 5e-6  # a condition, not a measurement: 2 x e_ref is the device's allowance, so a case whose own fp32 step strays further would swallow a real error
UNET = [c.name for c in T.CASES if c.backbone == "unet"]


def test_route_call_is_bound_and_declared():
    import os

    assert "ph_model_last_backward_routes" in L.SIGNATURES
    assert L.SIGNATURES["ph_model_last_backward_routes"] == L.SIGNATURES["ph_model_last_backward_kernels"]
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "posehip.h")) as f:
        header = f.read()
    assert "int ph_model_last_backward_routes(const ph_model* m, int32_t* routes, int32_t n_ops);" in header
    # the binding's constants are the header's
    defs = {k: int(eval(v, {})) for k, v in re.findall(r"^#define\s+PH_BR_(\w+)\s+(\(?[\d <()]+\)?)\s", header, re.M)}
    for name, value in defs.items():
        if name in ("PART_BITS",):
            assert L.BR_PART_BITS == value
        elif name.startswith(("WG_", "DG_")) or (name.startswith(("MASK_", "BIAS_")) and not name.endswith("SHIFT")):
            assert getattr(L, "BR_" + name) == value, name
    assert defs["MASK_SHIFT"] == L._BR_MASK_SHIFT and defs["BIAS_SHIFT"] == L._BR_BIAS_SHIFT and defs["ACCUMULATE"] == 1 << 10
    assert [defs[n] for n in ("FOLDED_MASK", "SUMMED_BIAS", "GELU_FUSED", "NO_LAUNCH")] == [1 << (L._BR_FLAG_SHIFT + i) for i in range(4)]
    assert {n[3:] for n in dir(L) if n.startswith(("BR_WG_", "BR_DG_", "BR_MASK_", "BR_BIAS_")) and isinstance(getattr(L, n), int)} == \
        {n for n in defs if n.startswith(("WG_", "DG_", "MASK_", "BIAS_")) and not n.endswith("SHIFT")}
    assert all(c < 32 for c in L.BR_DG_DMA_CODES) and all(c >= 32 for c in L.BR_DG_NAMES if c)


def test_route_words_round_trip():
    dgrads = list(L.BR_DG_NAMES) + list(L.BR_DG_DMA_CODES)
    seen = set()
    for i, (wg, dg) in enumerate(itertools.product(L.BR_WG_NAMES, dgrads)):
        f = dict(wgrad=(wg, (wg + 3) % len(L.BR_WG_NAMES)), dgrad=(dg, dgrads[(i * 7 + 1) % len(dgrads)]), accumulate=(i & 1, (i >> 1) & 1),
                 mask=i % len(L.BR_MASK_NAMES), bias=i % len(L.BR_BIAS_NAMES))
        f.update({name: (i >> (2 + j)) & 1 for j, name in enumerate(L.BR_FLAGS)})
        word = L.br_encode(**f)
        assert 0 <= word < 1 << 31  # an int32, sign bit clear
        assert L.br_decode(word) == f, f
        seen.add(word)
        assert L.br_dgrad_name(dg)
    assert len(seen) == len(L.BR_WG_NAMES) * len(dgrads)
    assert L.br_decode(0) == dict(wgrad=(0, 0), dgrad=(0, 0), accumulate=(0, 0), mask=0, bias=0, folded_mask=0, summed_bias=0, gelu_fused=0, no_launch=0)
    # each field alone lands in its own bits
    assert L.br_encode(wgrad=(0, L.BR_WG_WINO)) == L.BR_WG_WINO << L.BR_PART_BITS
    assert L.br_encode(dgrad=(L.BR_DG_GEMM5, 0), accumulate=(1, 0)) == (L.BR_DG_GEMM5 << 4) | (1 << 10)
    assert L.br_encode(no_launch=1) == 1 << 30


def test_table_is_well_formed():
    fields = set(L.br_decode(0))
    for c in T.CASES:
        assert 1 <= c.batch <= 3 and c.hw[0] <= 48 and c.hw[1] <= 64, c.name
        assert c.hw[0] % c.bb["max_stride"] == 0 and c.hw[1] % c.bb["max_stride"] == 0, c.name
        if c.backbone == "unet":
            assert 2 <= c.bb["max_stride"] <= 8, c.name
        assert c.measured is not None and c.floor is not None and 4 * c.measured <= c.floor <= 1e-4, c.name
        for sel, part, name, _value in c.must:
            assert name in fields and (part in (0, 1)) == (name in ("wgrad", "dgrad", "accumulate")), (c.name, name)


RELU_MARGIN = 1e-6  # ten times the ~1e-7 absolute error of a device forward on these nets (activations of order 1, fp32 sums of a few hundred terms)


@pytest.mark.parametrize("name", [c.name for c in T.CASES])
def test_no_relu_sits_on_its_kink(name):
    """A ReLU whose pre-activation lies within the forward's rounding of zero is on in one evaluation and off in another, and the gradients upstream of it then differ
    by whole terms -- between fp32 and float64 on the CPU as between the device and either (seed 5 of the narrow bottom-up net: one middle-block pre-activation of
    7e-9, and that conv's weight gradient 2.3e-3 of scale away on the device).  That is no property of a kernel: such a case gets another seed."""
    margin = T.relu_margin(T.BY_NAME[name])
    print(f"{name}: smallest |ReLU pre-activation| of the fp32 reference {margin:.2e}")
    assert margin >= RELU_MARGIN, margin


@pytest.mark.parametrize("name", UNET)
def test_unet_case_fp32_oracle_stays_close_to_float64_and_is_quick(name):
    case = T.BY_NAME[name]
    T.inputs(case)
    _l32, g32 = T.reference(case, False)
    T._REFS.pop((name, True), None)  # (time the step itself, not the table's cache)
    t0 = time.perf_counter()
    _l64, g64 = T.reference(case, True)
    took = time.perf_counter() - t0
    e_ref = T.e_rel(g32, g64)
    worst = max(e_ref, key=e_ref.get)
    print(f"{name}: fp32 oracle vs float64, worst tensor {worst} {e_ref[worst]:.2e}; float64 step {took:.2f} s")
    assert e_ref[worst] <= E_REF_CAP, (worst, e_ref[worst])
    assert took < 1.0, took
