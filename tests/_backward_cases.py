"""One table of tiny training steps, shared by tests/test_gpu_backward_routes.py (device gradients and the route record of ``ph_model_last_backward_routes``) and
tests/test_backward_routes_cpu.py (the references alone).  Each case names the routes of the reverse sweep it is there for (``must``); the device test reads them from the
record, never from a restated predicate, and then compares every gradient of that step with float64.

A ``must`` entry is ``(op selector, concat part or None, field of _lib.br_decode, value)``: at least one op whose ``OpSpec`` attributes equal the selector's shows that
value.  Selectors speak of the program (kind, channel counts), not of the router.

``measured`` is the worst ``e_hip`` of the case on an MI355X -- over all parameter tensors, |device gradient - float64 gradient| / the float64 tensor's largest magnitude --
and ``floor = 4 x measured`` (rounded up to two digits, never above the project's 1e-4) is what the device test allows where torch's own fp32 error does not allow
more: room for another compiler contracting sums differently, not for noise (the sweep is deterministic).  Both stand per case in ``MEASURED`` under the table.

Seeds are chosen on the CPU so that no ReLU of the reference sits on its kink (tests/test_backward_routes_cpu.py::test_no_relu_sits_on_its_kink) and, for the
class-vector case, so that torch's fp32 step agrees with float64 (seed 1 there: 3.4e-3 between the two CPU evaluations themselves).
"""
import contextlib
from dataclasses import dataclass, field
from typing import Optional

import torch

from oracle import cpu_ref as O
from sleap_nn_amd import _lib as L

CONV, INPUT, POOL, HEAD, CONVT, LINEAR, GELU, PATCH_CONV, PATCH_STEM = L.OP_CONV, L.OP_INPUT_CONV, L.OP_POOL, L.OP_HEAD, L.OP_CONVT, L.OP_LINEAR, L.OP_GELU, L.OP_PATCH_CONV, L.OP_PATCH_STEM


@dataclass
class Case:
    name: str
    backbone: str   # "unet" | "convnext" | "swint" | "pretrained"
    bb: dict
    heads: dict
    model_type: str
    batch: int
    hw: tuple
    seed: int
    options: dict = field(default_factory=dict)
    must: list = field(default_factory=list)
    module_kw: dict = field(default_factory=dict)
    frozen: bool = False             # the encoder ops run no step: their route words are 0
    measured: Optional[float] = None  # worst e_hip on the device
    floor: Optional[float] = None     # 4 x measured, at most 1e-4


def _unet(filters, rate, max_stride, output_stride=1, in_ch=1, **kw):
    bb = {"in_channels": in_ch, "kernel_size": 3, "filters": filters, "filters_rate": rate, "max_stride": max_stride, "stem_stride": None, "middle_block": True,
          "up_interpolate": True, "stacks": 1, "convs_per_block": 2, "output_stride": output_stride}
    bb.update(kw)
    return bb


def _single(n=2, stride=1):
    return {"confmaps": {"part_names": [f"n{i}" for i in range(n)], "output_stride": stride, "loss_weight": 1.0}}


def _bottomup(n=3, stride=1):
    names = [f"n{i}" for i in range(n)]
    return {"confmaps": {"part_names": names, "output_stride": stride, "loss_weight": 1.0},
            "pafs": {"edges": [[names[i], names[i + 1]] for i in range(n - 1)], "output_stride": stride * 2, "loss_weight": 0.7}}


def _unet_case(name, bb, batch, hw, seed, options=None, must=(), heads=None, mt="single_instance", **kw):
    return Case(name, "unet", bb, heads if heads is not None else _single(stride=bb["output_stride"]), mt, batch, hw, seed, dict(options or {}), list(must), **kw)


def _class_vector_case():
    bb = _unet(8, 1.5, 8, output_stride=2)
    heads = {"confmaps": {"part_names": ["A", "B"], "anchor_part": "A", "sigma": 1.5, "output_stride": 2, "loss_weight": 1.0},
             "class_vectors": {"classes": ["f", "m", "x"], "num_fc_layers": 2, "num_fc_units": 32, "global_pool": True, "output_stride": 8, "loss_weight": 0.3}}
    return Case("class_vector_head", "unet", bb, heads, "multi_class_topdown", 3, (40, 56), 4,
                must=[({"kind": LINEAR, "flags": L.FLAG_RELU}, None, "mask", L.BR_MASK_OWN), ({"kind": LINEAR, "flags": L.FLAG_RELU}, None, "bias", L.BR_BIAS_WITH_MASK),
                      ({"kind": LINEAR}, 0, "wgrad", L.BR_WG_ROW_GEMM), ({"kind": LINEAR}, 0, "dgrad", L.BR_DG_GEMM0)])


def _convnext_case(name, fuse):
    from tests.test_gpu_convnext import _bb

    bb = _bb(arch={"depths": [1, 1, 1, 1], "channels": [16, 32, 64, 128]}, stem_patch_stride=2, output_stride=2, in_channels=1)
    heads = {"confmaps": {"part_names": ["a", "b", "c"], "sigma": 2.5, "output_stride": 2, "loss_weight": 1.0, "anchor_part": None}}
    must = [({"kind": LINEAR}, None, "gelu_fused", fuse), ({"kind": GELU}, None, "no_launch", fuse), ({"kind": LINEAR}, 0, "wgrad", L.BR_WG_ROW_GEMM),
            ({"kind": PATCH_CONV}, 0, "dgrad", L.BR_DG_GEMM0), ({"kind": PATCH_STEM}, 0, "wgrad", L.BR_WG_PATCH_STEM), ({"kind": LINEAR}, None, "bias", L.BR_BIAS_ROW_WGRAD)]
    return Case(name, "convnext", bb, heads, "centered_instance", 2, (32, 64), 13, {"fuse_gelu_bwd": fuse}, must)


def _swin_case():
    from tests.test_gpu_swint_train import _bb, _heads

    bb = _bb(arch={"embed": 32, "depths": [1, 1, 1, 1], "num_heads": [1, 2, 4, 8]})
    return Case("swin_one_block_per_stage", "swint", bb, _heads(3), "single_instance", 2, (32, 64), 7,
                must=[({"kind": LINEAR}, 0, "wgrad", L.BR_WG_ROW_GEMM), ({"kind": LINEAR}, None, "gelu_fused", 1), ({"kind": LINEAR, "bias": None}, None, "bias", L.BR_BIAS_NONE)],
                module_kw={"swint_training": True, "stochastic_depth_prob": 0.0})


def _convnextv2_case():
    from tests.test_pretrained_cpu import bb_of, heads_of, hf_dir

    return Case("convnextv2_frozen_encoder", "pretrained", bb_of("A", hf_dir("A", None)), heads_of("A"), "single_instance", 2, (32, 64), 78, frozen=True,
                must=[({"kind": CONV}, 0, "wgrad", L.BR_WG_WINO)], module_kw={"pretrained_training": True, "freeze_encoder": True})


W16 = _unet(16, 1, 4)            # every conv 16 -> 16, decoder parts 16 + 16
F16R2 = _unet(16, 2, 2)          # 16 | 32 | decoder conv (16 + 32) -> 16
F24 = _unet(24, 1.5, 4)          # 24 | 36 | 54: padded widths 32 | 48 | 64
F12 = _unet(12, 1.5, 8, output_stride=2)  # 12 | 18 | 27 | 40
F8 = _unet(8, 2, 8)
WIDE = _unet(32, 2, 4)          # 32 | 64 | 128

CASES = [
    # ---- weight gradient
    _unet_case("wgrad16_wino_16_to_16", W16, 2, (36, 52), 2, must=[({"kind": CONV, "cin0": 16, "cin1": 0, "cout": 16}, 0, "wgrad", L.BR_WG_WINO16), ({"kind": CONV}, 0, "dgrad", L.KV_W16)]),
    _unet_case("wgrad_wino_ragged_cout", F12, 2, (40, 56), 11, heads=_bottomup(3, 2), mt="bottomup",
               must=[({"kind": CONV, "cout": 18}, 0, "wgrad", L.BR_WG_WINO), ({"kind": CONV, "cout": 27}, 0, "wgrad", L.BR_WG_WINO), ({"kind": CONV, "cout": 40}, 0, "wgrad", L.BR_WG_WINO)]),
    _unet_case("wgrad_wino_second_part_and_cp48", F24, 2, (36, 52), 4,
               must=[({"kind": CONV, "cin0": 36, "cin1": 54, "cout": 36}, 1, "wgrad", L.BR_WG_WINO), ({"kind": CONV, "cin0": 36, "cin1": 54, "cout": 36}, 0, "wgrad", L.BR_WG_WINO),
                     ({"kind": POOL}, None, "folded_mask", 1), ({"kind": POOL}, None, "summed_bias", 0), ({"kind": POOL}, None, "summed_bias", 1)]),
    _unet_case("wgrad_direct_32_to_16_part", F16R2, 2, (26, 36), 1,
               must=[({"kind": CONV, "cin0": 16, "cin1": 32, "cout": 16}, 1, "wgrad", L.BR_WG_DIRECT), ({"kind": CONV, "cin0": 16, "cin1": 32, "cout": 16}, 0, "wgrad", L.BR_WG_WINO16)]),
    _unet_case("wgrad_direct_everywhere", F16R2, 2, (26, 36), 1, {"wgrad_wino": 0},
               must=[({"kind": CONV, "cin0": 16, "cin1": 32, "cout": 16}, 0, "wgrad", L.BR_WG_DIRECT), ({"kind": CONV, "cin0": 32, "cout": 32}, 0, "wgrad", L.BR_WG_DIRECT)]),
    _unet_case("wgrad_rows_auto_128", _unet(128, 1, 2), 1, (12, 16), 1, {"wgrad_rows": 1}, must=[({"kind": CONV, "cin0": 128, "cin1": 0, "cout": 128}, 0, "wgrad", L.BR_WG_ROWS9)]),
    _unet_case("wgrad_below_rows_bar_96", _unet(96, 1, 2), 1, (12, 16), 1, {"wgrad_rows": 1},
               must=[({"kind": CONV, "cin0": 96, "cin1": 0, "cout": 96}, 0, "wgrad", L.BR_WG_WINO), ({"kind": POOL}, None, "folded_mask", 1), ({"kind": POOL}, None, "summed_bias", 0)]),
    _unet_case("wgrad_rows_forced_narrow", F8, 2, (40, 56), 9, {"wgrad_rows": 2}, must=[({"kind": CONV, "cin0": 8, "cout": 8}, 0, "wgrad", L.BR_WG_ROWS9)]),
    # ---- data gradient
    # (conv3x3_route: the wave-private kernel, F(2x2,3x3), F(2,3) along x or, under dgrad_wino = 0, the direct kernel; conv3x3_c16 once conv_w16 is off)
    _unet_case("dgrad_default_narrow", F8, 3, (40, 56), 12, heads=_bottomup(3, 1), mt="bottomup", must=[({"kind": CONV}, 0, "dgrad", L.KV_W16), ({"kind": CONV}, 0, "accumulate", 0)]),
    _unet_case("dgrad_default_wide", WIDE, 2, (20, 28), 8, must=[({"kind": CONV}, 0, "dgrad", L.KV_W16), ({"kind": CONV}, 0, "dgrad", L.KV_WINO2D), ({"kind": CONV}, 0, "dgrad", L.KV_WINO1D),
                                                                  ({"kind": CONV}, 1, "dgrad", L.KV_WINO2D)]),
    _unet_case("dgrad_c16_route0", W16, 2, (36, 52), 2, {"conv_w16": 0}, must=[({"kind": CONV, "cin0": 16, "cin1": 0, "cout": 16}, 0, "dgrad", L.KV_C16)]),
    _unet_case("dgrad_wino4_everywhere", _unet(64, 1, 2), 2, (20, 28), 10, {"conv_wino4": 3}, must=[({"kind": CONV}, 0, "dgrad", L.KV_WINO4)]),
    _unet_case("dgrad_no_w16_no_wino2d", WIDE, 2, (20, 28), 8, {"conv_w16": 0, "conv_wino2d": 0, "conv_c16": 0}, must=[({"kind": CONV}, 0, "dgrad", L.KV_WINO1D)]),
    _unet_case("dgrad_register_staged_all", F16R2, 2, (26, 36), 1, {"conv_dma": 0}, must=[({"kind": CONV, "cin0": 32, "cout": 32}, 0, "dgrad", L.BR_DG_REGSTAGED)]),
    _unet_case("dgrad_register_staged_narrow", F16R2, 2, (26, 36), 1, {"conv_dma32": 0}, must=[({"kind": CONV}, 0, "dgrad", L.BR_DG_REGSTAGED)]),
    _unet_case("dgrad_direct_kernels", WIDE, 2, (20, 28), 8, {"dgrad_wino": 0}, must=[({"kind": CONV}, 0, "dgrad", L.KV_DIRECT)]),
    # ---- mask and bias
    _unet_case("mask_fold_on", W16, 2, (36, 52), 2, {"mask_fold": 1}, heads=_bottomup(3, 1), mt="bottomup",
               must=[({"kind": POOL}, None, "folded_mask", 1), ({"kind": HEAD}, None, "folded_mask", 1), ({"kind": CONV}, None, "folded_mask", 1), ({"kind": CONV}, None, "mask", L.BR_MASK_EARLIER),
                     ({"kind": CONV}, None, "bias", L.BR_BIAS_CLOSER), ({"kind": INPUT}, None, "bias", L.BR_BIAS_INPUT_WGRAD)]),
    _unet_case("mask_fold_off", W16, 2, (36, 52), 2, {"mask_fold": 0}, heads=_bottomup(3, 1), mt="bottomup",
               must=[({"kind": POOL}, None, "folded_mask", 0), ({"kind": HEAD}, None, "folded_mask", 0), ({"kind": CONV}, None, "mask", L.BR_MASK_OWN), ({"kind": CONV}, None, "bias", L.BR_BIAS_WITH_MASK),
                     ({"kind": INPUT}, None, "mask", L.BR_MASK_OWN)]),
    _unet_case("cp48_head_and_pool", _unet(40, 1, 2), 2, (26, 36), 10, must=[({"kind": POOL}, None, "folded_mask", 1), ({"kind": POOL}, None, "summed_bias", 0), ({"kind": HEAD}, None, "folded_mask", 0),
                                                                             ({"kind": CONV}, None, "bias", L.BR_BIAS_OWN)]),
    # ---- other ops
    _unet_case("transposed_conv_decoder", _unet(8, 1.5, 8, output_stride=2, up_interpolate=False), 2, (40, 56), 6, heads=_bottomup(3, 2), mt="bottomup",
               must=[({"kind": CONVT}, 0, "accumulate", 1), ({"kind": CONVT}, 0, "accumulate", 0), ({"kind": CONVT}, 0, "wgrad", L.BR_WG_CONVT_TAPS), ({"kind": CONVT}, 0, "dgrad", L.BR_DG_GEMM4), ({"kind": CONVT}, None, "bias", L.BR_BIAS_WITH_MASK)]),
    _unet_case("k5_convs", _unet(8, 2, 4, in_ch=3, kernel_size=5), 2, (36, 52), 31,
               must=[({"kind": INPUT}, 0, "wgrad", L.BR_WG_PATCH_STEM), ({"kind": CONV}, 0, "wgrad", L.BR_WG_ROWSKK), ({"kind": CONV}, 1, "wgrad", L.BR_WG_ROWSKK), ({"kind": CONV}, 0, "dgrad", L.BR_DG_GEMM5),
                     ({"kind": CONV}, 0, "accumulate", 0)]),
    _class_vector_case(),
    _convnext_case("convnext_gelu_fused", 1),
    _convnext_case("convnext_gelu_unfused", 0),
    _swin_case(),
    _convnextv2_case(),
]
# worst e_hip of each case on an MI355X (ROCm 7 hipcc, gfx950), and its floor = 4 x that, rounded up to two digits
MEASURED = {
    "wgrad16_wino_16_to_16": (2.212e-07, 8.9e-07),
    "wgrad_wino_ragged_cout": (2.427e-07, 9.8e-07),
    "wgrad_wino_second_part_and_cp48": (2.443e-07, 9.8e-07),
    "wgrad_direct_32_to_16_part": (2.668e-07, 1.1e-06),
    "wgrad_direct_everywhere": (1.957e-07, 7.9e-07),
    "wgrad_rows_auto_128": (2.520e-07, 1.1e-06),
    "wgrad_below_rows_bar_96": (2.070e-07, 8.3e-07),
    "wgrad_rows_forced_narrow": (3.891e-07, 1.6e-06),
    "dgrad_default_narrow": (3.197e-07, 1.3e-06),
    "dgrad_default_wide": (2.434e-07, 9.8e-07),
    "dgrad_c16_route0": (2.083e-07, 8.4e-07),
    "dgrad_wino4_everywhere": (3.891e-07, 1.6e-06),
    "dgrad_no_w16_no_wino2d": (2.027e-07, 8.2e-07),
    "dgrad_register_staged_all": (1.848e-07, 7.4e-07),
    "dgrad_register_staged_narrow": (1.848e-07, 7.4e-07),
    "dgrad_direct_kernels": (2.194e-07, 8.8e-07),
    "mask_fold_on": (2.099e-07, 8.4e-07),
    "mask_fold_off": (2.099e-07, 8.4e-07),
    "cp48_head_and_pool": (2.472e-07, 9.9e-07),
    "transposed_conv_decoder": (2.683e-07, 1.1e-06),
    "k5_convs": (1.534e-07, 6.2e-07),
    "class_vector_head": (3.801e-07, 1.6e-06),
    "convnext_gelu_fused": (8.937e-07, 3.6e-06),
    "convnext_gelu_unfused": (8.937e-07, 3.6e-06),
    "swin_one_block_per_stage": (1.688e-06, 6.8e-06),
    "convnextv2_frozen_encoder": (4.462e-07, 1.8e-06),
}
for _c in CASES:
    _c.measured, _c.floor = MEASURED[_c.name]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


# ---- inputs and references

@contextlib.contextmanager
def _float64_images():
    """The restatements of tests/swin_ref.py and tests/convnextv2_ref.py normalise the image to fp32 (O.normalize_input); for their float64 step the normalised image is
    widened, as oracle.cpu_ref.model_forward does for float64 weights."""
    orig = O.normalize_input
    O.normalize_input = lambda x: orig(x).double()
    try:
        yield
    finally:
        O.normalize_input = orig


_INPUTS = {}


def inputs(case):
    """(state dict, image, targets, loss weights) of a case, built once: UNets as tests/test_gpu_training.py::_setup builds them, the others as their own train tests do."""
    if case.name in _INPUTS:
        return _INPUTS[case.name]
    bb, heads, mt, seed = case.bb, case.heads, case.model_type, case.seed
    g = torch.Generator().manual_seed(seed)
    shape = (case.batch, bb["in_channels"], case.hw[0], case.hw[1])
    if case.backbone == "unet" and "class_vectors" in heads:  # (O.init_state knows map heads only: drawn over the model's own shapes, as test_multiclass_topdown_training_matches_autograd does)
        from sleap_nn_amd.architectures.model import Model

        sd = {}
        for k, s in Model("unet", bb, heads, mt).param_shapes.items():
            fan = 1
            for d in s[1:]:
                fan *= int(d)
            sd[k] = (torch.rand(s, generator=g) * 2 - 1) * (1.5 / fan ** 0.5 if len(s) > 1 else 0.1)
        img = torch.randint(0, 256, shape, dtype=torch.uint8, generator=g)
        ref_out = O.model_forward(sd, bb, heads, mt, img)
    elif case.backbone == "unet":
        sd = O.init_state(bb, heads, mt, seed=seed, head_scale=1.0)
        for k in sd:
            if k.endswith(".bias"):
                sd[k] = (torch.rand(sd[k].shape, generator=g) - 0.5) * 0.2
        img = torch.randint(0, 256, shape, dtype=torch.uint8, generator=g)
        ref_out = O.model_forward(sd, bb, heads, mt, img)
    elif case.backbone == "convnext":
        sd = O.init_state_convnext(bb, heads, mt, seed=seed, head_scale=1.0, layer_scale=0.6, randomize_affine=True)
        img = torch.randint(0, 256, shape, dtype=torch.uint8, generator=g)
        ref_out = O.model_forward(sd, bb, heads, mt, img, backbone="convnext")
    elif case.backbone == "swint":
        from tests import swin_ref as R

        sd = R.init_state_swint(bb, heads, mt, seed=seed)
        img = torch.randint(0, 256, shape, dtype=torch.uint8, generator=g)
        with torch.no_grad():
            ref_out = R.model_forward(sd, bb, heads, mt, img)
    else:
        from tests import convnextv2_ref as R
        from tests.test_pretrained_cpu import golden

        sd = golden("A")[1]
        img = torch.randint(0, 256, shape, dtype=torch.uint8, generator=g)
        with torch.no_grad():
            ref_out = R.model_forward(sd, bb, heads, mt, img)
    if "ClassVectorsHead" in ref_out:
        n = ref_out["ClassVectorsHead"].shape[1]
        targets = {k: (torch.nn.functional.one_hot(torch.randint(0, n, (case.batch,), generator=g), n).float() if k == "ClassVectorsHead" else torch.rand(v.shape, generator=g) * 0.5)
                   for k, v in ref_out.items()}
    else:
        targets = {k: torch.rand(v.shape, generator=g) * 0.5 for k, v in ref_out.items()}
    lw = [float(heads[key].get("loss_weight", 1.0)) for _h, key in O.HEAD_ORDER[mt]]
    _INPUTS[case.name] = (sd, img, targets, lw)
    return _INPUTS[case.name]


def relu_margin(case):
    """Smallest |pre-activation| over every ReLU of the case's fp32 reference forward (the references call ``F.relu``)."""
    import torch.nn.functional as F

    sd, img, _targets, _lw = inputs(case)
    relu, least = F.relu, []

    def watched(x, *a, **k):
        least.append(float(x.detach().abs().min()))
        return relu(x, *a, **k)

    F.relu = watched
    try:
        with torch.no_grad():
            if case.backbone in ("unet", "convnext"):
                O.model_forward(sd, case.bb, case.heads, case.model_type, img, backbone=case.backbone)
            elif case.backbone == "swint":
                from tests import swin_ref as R

                R.model_forward(sd, case.bb, case.heads, case.model_type, img)
            else:
                from tests import convnextv2_ref as R

                R.model_forward(sd, case.bb, case.heads, case.model_type, img)
    finally:
        F.relu = relu
    return min(least)


_REFS = {}


def reference(case, double):
    """(losses [total, heads...], {parameter: gradient}) of the case's step in fp32 (``double`` False) or float64, computed once and shared."""
    key = (case.name, bool(double))
    if key in _REFS:
        return _REFS[key]
    sd, img, targets, lw = inputs(case)
    if double:
        sd = {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
        targets = {k: v.double() for k, v in targets.items()}
    bb, heads, mt = case.bb, case.heads, case.model_type
    if case.backbone == "unet":
        out = O.training_step(sd, bb, heads, mt, img, targets, lw)
    elif case.backbone == "convnext":
        out = O.training_step(sd, bb, heads, mt, img, targets, lw, backbone="convnext")
    elif case.backbone == "swint":
        from tests.test_gpu_swint_train import _ref_step

        with (_float64_images() if double else contextlib.nullcontext()):
            loss, grads, _out = _ref_step(sd, bb, heads, mt, img, targets)
        out = ([loss, loss], grads)
    else:
        from tests.test_gpu_pretrained_train import _ref_step

        with (_float64_images() if double else contextlib.nullcontext()):
            loss, grads, *_ = _ref_step(sd, bb, heads, img, targets, frozen=case.frozen, mt=mt)
        out = ([loss, loss], grads)
    _REFS[key] = out
    return out


def module(case, device):
    """The case's TrainingModule on ``device`` with the case's options set."""
    from sleap_nn_amd.architectures.model import Model
    from sleap_nn_amd.training.module import TrainingModule

    sd, _img, _targets, lw = inputs(case)
    m = Model(case.backbone, case.bb, case.heads, case.model_type)
    m.load_state_dict(sd)
    tm = TrainingModule(m, device, loss_weights=lw, **case.module_kw)
    for k, v in case.options.items():
        tm.model.set_option(k, v)
    return tm


def matches(op, selector):
    return all(getattr(op, k) == v for k, v in selector.items())


def field_of(word, part, name):
    v = L.br_decode(word)[name]
    return v[part] if part is not None else v


def e_rel(got, ref64):
    """Per tensor: largest |got - float64| over the float64 tensor's largest magnitude (the rule of test_backward_cfg3_network_with_interior_tiles)."""
    return {k: float((got[k].double() - r).abs().max()) / max(float(r.abs().max()), 1e-30) for k, r in ref64.items()}
