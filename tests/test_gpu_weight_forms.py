"""Every weight form of a handle follows ``ph_model_set_params``: a handle created from weights A and re-bound to the arena of weights B must hold, allocation by
allocation (``ph_model_debug_allocs``), the bytes of a handle created from B.  That holds the gather maps, every derived launch (csrc/weights.hip: the table of derived
forms, ``refresh``) and the GRN bias fold to the create-time packers, and it covers the forms no default route reads.

The second case walks the stale path: on a handle with ``workspace_reuse`` 0 and exact precision ``ph_model_set_params`` leaves the forms only inference plans read
(F(4x4,3x3), small-map) and the fp16 row-GEMM images at A -- exactly those, counted here from the program --, and the next forward that can read them refreshes them.

Models and frames are those of tools/weights_trace.py (64 x 96, batch 2).

One exception, as the code stood before the forms got their table: a ConvNeXtV2 program has no fp16 form (forward_format is fp32 whatever the options say), so no forward
of it reads -- or refreshes -- its stale fp16 row-GEMM images (``PackedOp::w_cnx_f16_dev`` of each Linear / 2x2 conv); ``ph_model_set_params`` under fp16 + ``convnext_f16``
does refresh them (first case)."""
import ctypes as C

import pytest
import torch

from sleap_nn_amd import _lib as L
from tools.forward_trace import DEV, convnext_cfg, convnextv2_cfg, image, make, swin_cfg, unet_cfg

pytestmark = pytest.mark.gpu
HW = (64, 96)
MODELS = {
    "unet bilinear": ("unet", lambda: unet_cfg("bilinear"), 1, None),
    "unet transposed": ("unet", lambda: unet_cfg("transposed"), 1, None),
    "unet k5": ("unet", lambda: unet_cfg("k5"), 1, None),
    "convnext 96": ("convnext", lambda: convnext_cfg([96, 192, 384, 768]), 1, "convnext_f16"),
    "swint small": ("swint", swin_cfg, 1, "swint_f16"),
    "convnextv2 tiny": ("pretrained", convnextv2_cfg, 3, "convnext_f16"),
}
_reference = {}


def _pad16(n):
    return (n + 15) // 16 * 16


def _handle(name, seed):
    """A model created from the weights of ``seed`` after one forward each at exact, split and fp16 precision (the lazy fp16 packs exist), back at exact."""
    backbone, cfg, channels, f16_option = MODELS[name]
    m = make(backbone, *cfg(), seed)
    img = image(2, channels, HW, 7)
    m(img)
    m.set_precision("split")(img)
    m.set_precision("fp16", **({f16_option: True} if f16_option else {}))(img)
    if f16_option:
        m.set_option(f16_option, 0)
    m.set_precision("exact")
    return m, img


def _bytes_of(name, seed):
    """(allocation count, bytes of every allocation) of the handle created from ``seed``; computed once per model and left unchanged."""
    if (name, seed) not in _reference:
        m, _ = _handle(name, seed)
        n0 = len(m.debug_allocs())
        _reference[(name, seed)] = (n0, m.debug_allocs(read_first=n0))
    return _reference[(name, seed)]


def _set_params(m, flat_dev):
    L.check(L.lib().ph_model_set_params(m._handle, C.c_void_p(flat_dev.data_ptr()), L.current_stream_ptr()))


def _differing(got, want):
    return [i for i, (g, w) in enumerate(zip(got, want)) if g.shape != w.shape or not torch.equal(g, w)]


def _stale_forms(m):
    """How many forms ``ph_model_set_params`` may leave stale on a handle with ``workspace_reuse`` 0 at exact precision, from the program alone: per 3x3 conv one
    small-map form; one F(4x4,3x3) form where the layer has an N tile of 64 (>= 64 padded output channels, or exactly 32 with the second N-tile-64 packing) and >= 64
    padded input channels, and one per concat source whose data-gradient conv has those shapes (outputs = the source's channels, inputs = the layer's outputs); one fp16
    image per Linear / 2x2-stride-2 conv."""
    wino4 = smallmap = images = 0
    for op in m.ops:
        if op.kind == L.OP_CONV and op.ksize == 3:
            cinp = _pad16(op.cin0) + (_pad16(op.cin1) if op.cin1 > 0 else 0)
            smallmap += 1
            wino4 += int((_pad16(op.cout) >= 64 or _pad16(op.cout) == 32) and cinp >= 64)
            wino4 += sum(int(part > 0 and _pad16(part) >= 64 and _pad16(op.cout) >= 64) for part in (op.cin0, op.cin1))
        images += int(op.kind in (L.OP_LINEAR, L.OP_PATCH_CONV))
    return wino4 + smallmap, images


@pytest.mark.parametrize("name", list(MODELS))
def test_set_params_leaves_every_allocation_as_a_fresh_handle_has_it(name):
    f16_option = MODELS[name][3]
    n0, want = _bytes_of(name, 22)
    m, _ = _handle(name, 21)
    assert len(m.debug_allocs()) == n0
    assert _differing(m.debug_allocs(read_first=n0), want), "weights A and B pack to the same bytes: the case would be vacuous"
    m.set_option("workspace_reuse", 1)
    if f16_option:
        m.set_precision("fp16", **{f16_option: True})
    _set_params(m, make(MODELS[name][0], *MODELS[name][1](), 22).flat_params().to(DEV))
    assert _differing(m.debug_allocs(read_first=n0), want) == []


@pytest.mark.parametrize("name", list(MODELS))
def test_forms_left_stale_hold_the_old_weights_until_a_forward_that_reads_them(name):
    f16_option = MODELS[name][3]
    n0, want = _bytes_of(name, 22)
    _, old = _bytes_of(name, 21)
    m, img = _handle(name, 21)
    m.set_option("workspace_reuse", 0)
    _set_params(m, make(MODELS[name][0], *MODELS[name][1](), 22).flat_params().to(DEV))
    got = m.debug_allocs(read_first=n0)
    stale = _differing(got, want)
    inference_only, images = _stale_forms(m)
    print(f"{name}: {n0} allocations, {len(stale)} left stale (expected {inference_only} inference-only forms + {images} fp16 images)")
    assert all(torch.equal(got[i], old[i]) for i in stale), "an allocation holds neither the old nor the new weights"
    assert len(stale) == inference_only + images
    m.set_option("workspace_reuse", 1)
    if f16_option:
        m.set_precision("fp16", **{f16_option: True})
    m(img)
    after = m.debug_allocs(read_first=n0)
    left = _differing(after, want)
    if name == "convnextv2 tiny":  # (no fp16 form: see the module docstring)
        assert len(left) == images and set(left) <= set(stale) and all(torch.equal(after[i], old[i]) for i in left)
    else:
        assert left == []
