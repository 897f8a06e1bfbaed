"""One table of tiny UNet forwards in the plain-fp16 precision, shared by tests/test_gpu_f16_emulation.py (the device against tests/_f16_emulation.py) and
tests/test_f16_emulation_cpu.py (the emulation against the oracle and against a torch-fp32 stand-in).  Each case names the kernel forms it is there for (``must``); the
device test reads them from ``last_kernels()`` / ``last_rows_plans()`` of the case's forwards, never from a restated predicate.

A ``must`` entry is one of
  ("kv", code)                     some op of the keep-everything or of the inference forward reports that PH_KV_* code
  ("rows", aligned, MT, MG)        some op ran that instantiation of conv3x3_f16_rows_kernel (aligned = Wt % 16 == 0; from last_rows_plans())
  ("persist", "64" | "32" | "64+head")  some op on PH_KV_F16 of that N tile (the library's N tile is 64 from 64 padded output channels on, read off the op's ``cout``), "+head": the
                                   head behind it reports PH_KV_FUSED

``pin`` is the handle option conv_f16_rows_pin as (R, Wt, MG).  Maps are at most 48 x 64 and batches 1 to 3: a case is a few seconds, most of it the float64 convolutions.

``MEASURED`` under the table holds, per case, what an MI355X gave: the worst |d - r| / e over the elements with e > 0 (at most 1 by the bound) and the worst share of
elements with d != r over the case's fp16 tensors; ``floor = 4 x`` that share, never above ``SHARE_CAP``.
"""
from dataclasses import dataclass, field
from typing import Optional

import torch

from oracle import cpu_ref as O
from sleap_nn_amd import _lib as L

SHARE_CAP = 0.01       # a condition, not a measurement: no tensor may differ from the emulation's value in more than 1 % of its elements
STANDIN_SHARE = 0.0025  # what the CPU test holds the torch-fp32 stand-in to, so that the cap is never what lets a case pass


@dataclass
class Case:
    name: str
    bb: dict
    heads: dict
    model_type: str
    batch: int
    hw: tuple
    seed: int
    options: dict = field(default_factory=dict)
    pin: Optional[tuple] = None
    must: list = field(default_factory=list)
    float_frames: bool = False
    measured: Optional[tuple] = None
    floor: Optional[float] = None


def _unet(filters, rate, max_stride, output_stride=1, in_ch=1, **kw):
    bb = {"in_channels": in_ch, "kernel_size": 3, "filters": filters, "filters_rate": rate, "max_stride": max_stride, "stem_stride": None, "middle_block": True,
          "up_interpolate": True, "stacks": 1, "convs_per_block": 2, "output_stride": output_stride}
    bb.update(kw)
    return bb


def _single(n, stride):
    return {"confmaps": {"part_names": [f"n{i}" for i in range(n)], "output_stride": stride}}, "single_instance"


def _bottomup(n, stride):
    names = [f"n{i}" for i in range(n)]
    return {"confmaps": {"part_names": names, "output_stride": stride}, "pafs": {"edges": [[names[i], names[i + 1]] for i in range(n - 1)], "output_stride": 2 * stride}}, "bottomup"


def _multiclass(n, stride):
    return {"confmaps": {"part_names": [f"n{i}" for i in range(n)], "output_stride": stride}, "class_maps": {"classes": ["a", "b", "c"], "output_stride": 2 * stride}}, "multi_class_bottomup"


def _case(name, bb, heads_mt, batch, hw, seed, options=None, pin=None, must=(), **kw):
    return Case(name, bb, heads_mt[0], heads_mt[1], batch, hw, seed, dict(options or {}), pin, list(must), **kw)


N64 = _unet(64, 1, 2)        # input conv 1 -> 64 | 64 -> 64 + pool | middle 64 | bilinear, (64 + 64) -> 64, 64 -> 64 | head on a 64-channel producer
N128 = _unet(128, 1, 2)      # the same at 128 channels: the N tile of 128 (MG 2), a head on a 128-channel producer
ROWS = {"conv_f16_rows": 2}
NO_ROWS = {"conv_f16_rows": 0}

CASES = [
    # ---- conv3x3_f16_persist_kernel
    _case("persist_narrow_ragged", _unet(24, 1.5, 4), _single(17, 1), 1, (52, 44), 3, NO_ROWS,
          must=[("persist", "32"), ("persist", "64"), ("kv", L.KV_F16)]),  # 24 | 36 | 54 channels: Cin padded to a 32 chunk, N tiles not full, two sources 36 + 54 and 24 + 36; maps 52 x 44, 26 x 22, 13 x 11; the head on 24 channels is not fused
    _case("persist_odd_pool", _unet(24, 1.5, 4, output_stride=4), _single(17, 4), 2, (26, 22), 4, NO_ROWS,
          must=[("persist", "32"), ("persist", "64+head")]),  # no decoder: 13 x 11 pooled to 7 x 6 in the conv's epilogue (zero padding), 17 head channels on the 54-channel middle block
    _case("persist_cin16_cin48", _unet(16, 3, 2), _single(3, 1), 2, (20, 36), 5, NO_ROWS,
          must=[("persist", "32"), ("persist", "64"), ("kv", L.KV_STEM)]),  # Cin 16 (half-empty chunk) and 48, two sources 16 + 48; the map cuts the 16 x 32 tile both ways
    _case("persist_two_n_tiles_64_128", _unet(64, 2, 2), _single(1, 1), 1, (20, 36), 7, NO_ROWS,
          must=[("persist", "64"), ("persist", "64+head")]),  # Cout 128 (two N tiles), two sources 64 + 128, a 1-channel head in the epilogue
    _case("persist_heads_17_32", _unet(64, 1, 4), _bottomup(17, 1), 1, (24, 40), 9, NO_ROWS, must=[("persist", "64+head"), ("kv", L.KV_FUSED)]),  # 17 and 32 head channels, both fused
    _case("persist_head_33_standalone", N64, _single(33, 1), 2, (26, 22), 11, NO_ROWS, must=[("persist", "64")]),  # 33 head channels: head1x1_mfma_kernel; the middle block on 13 x 11, smaller than one tile
    _case("persist_pool_only_store", _unet(64, 1, 4, output_stride=2), _single(2, 2), 2, (28, 36), 13, NO_ROWS, must=[("persist", "64")]),  # enc0's full-resolution output is nobody's skip: skip_dst in the inference plan
    # ---- conv3x3_f16_rows_kernel, every instantiation: ALIGNED x MG 4 (R x Wt pixels over 4 x 16 MT)
    _case("rows_a_mt3_mg4", N64, _single(2, 1), 1, (20, 16), 21, ROWS, pin=(12, 16, 4), must=[("rows", True, 3, 4), ("kv", L.KV_F16_ROWS)]),   # partial last tile in H
    _case("rows_a_mt4_mg4", N64, _single(2, 1), 1, (20, 32), 22, ROWS, pin=(16, 16, 4), must=[("rows", True, 4, 4)]),   # column strips (W 32 > Wt 16)
    _case("rows_a_mt5_mg4", N64, _single(2, 1), 2, (12, 40), 23, ROWS, pin=(10, 32, 4), must=[("rows", True, 5, 4)]),   # partial last tile in W (40 = 32 + 8) and in H
    _case("rows_a_mt6_mg4", N64, _single(17, 1), 1, (20, 32), 24, ROWS, pin=(12, 32, 4), must=[("rows", True, 6, 4), ("kv", L.KV_FUSED)]),  # fused head on the 64-channel producer
    _case("rows_a_mt7_mg4", N64, _single(2, 1), 1, (16, 32), 25, ROWS, pin=(14, 32, 4), must=[("rows", True, 7, 4)]),
    _case("rows_a_mt8_mg4", N64, _single(2, 1), 1, (20, 32), 26, ROWS, pin=(16, 32, 4), must=[("rows", True, 8, 4)]),
    _case("rows_a_mt9_mg4", N64, _single(2, 1), 1, (20, 48), 27, ROWS, pin=(12, 48, 4), must=[("rows", True, 9, 4)]),
    # ALIGNED x MG 2 (Cout a multiple of 128; R x Wt pixels over 2 x 16 MT)
    _case("rows_a_mt3_mg2", N128, _single(2, 1), 1, (10, 32), 31, ROWS, pin=(6, 16, 2), must=[("rows", True, 3, 2)]),
    _case("rows_a_mt4_mg2", N128, _single(2, 1), 1, (10, 16), 32, ROWS, pin=(8, 16, 2), must=[("rows", True, 4, 2)]),
    _case("rows_a_mt5_mg2", N128, _single(2, 1), 1, (12, 16), 33, ROWS, pin=(10, 16, 2), must=[("rows", True, 5, 2)]),
    _case("rows_a_mt6_mg2", N128, _single(32, 1), 1, (14, 16), 34, ROWS, pin=(12, 16, 2), must=[("rows", True, 6, 2), ("kv", L.KV_FUSED)]),  # fused head on the 128-channel producer
    _case("rows_a_mt7_mg2", N128, _single(2, 1), 1, (16, 16), 35, ROWS, pin=(14, 16, 2), must=[("rows", True, 7, 2)]),
    _case("rows_a_mt8_mg2", N128, _single(2, 1), 1, (20, 16), 36, ROWS, pin=(16, 16, 2), must=[("rows", True, 8, 2)]),
    _case("rows_a_mt9_mg2", N128, _single(2, 1), 1, (20, 16), 37, ROWS, pin=(18, 16, 2), must=[("rows", True, 9, 2)]),
    # not ALIGNED (per-lane fragment addresses): whole rows of 22, 26, 44 pixels
    _case("rows_u_mt3_mg4", N64, _single(2, 1), 2, (12, 22), 41, ROWS, pin=(8, 22, 4), must=[("rows", False, 3, 4)]),
    _case("rows_u_mt4_mg4", N64, _single(2, 1), 1, (12, 26), 42, ROWS, pin=(8, 26, 4), must=[("rows", False, 4, 4)]),
    _case("rows_u_mt5_mg4", N64, _single(2, 1), 1, (10, 44), 43, ROWS, pin=(6, 44, 4), must=[("rows", False, 5, 4)]),
    _case("rows_u_mt3_mg2", N128, _single(2, 1), 1, (10, 22), 44, ROWS, pin=(4, 22, 2), must=[("rows", False, 3, 2)]),
    _case("rows_u_mt4_mg2", N128, _single(2, 1), 1, (10, 26), 45, ROWS, pin=(4, 26, 2), must=[("rows", False, 4, 2)]),
    _case("rows_u_mt5_mg2", N128, _single(2, 1), 1, (12, 22), 46, ROWS, pin=(6, 22, 2), must=[("rows", False, 5, 2)]),
    # the row-tile kernel's other forms: the folded bilinear in both arithmetics (inference plan; H and W even, image borders inside the tile), pool-only store,
    # a workgroup that walks more than one tile (288 tiles of 2 x 16 pixels at batch 3 on at most 256 workgroups)
    _case("rows_lowres_f16math", _unet(64, 1, 4), _bottomup(3, 1), 1, (24, 40), 51, ROWS, must=[("kv", L.KV_F16_ROWS)]),
    _case("rows_lowres_fp32math", _unet(64, 1, 4), _bottomup(3, 1), 1, (24, 40), 52, {"conv_f16_rows": 2, "upsample_f16math": 0}, must=[("kv", L.KV_F16_ROWS)]),
    _case("rows_pool_only_store", _unet(64, 1, 4, output_stride=2), _single(2, 2), 2, (28, 36), 53, ROWS, must=[("kv", L.KV_F16_ROWS)]),
    _case("rows_many_tiles", N64, _single(2, 1), 3, (48, 64), 54, ROWS, pin=(2, 16, 4), must=[("rows", True, 3, 4)]),
    # ---- block2_c32_f16_kernel and stem_f16_kernel (inference plans; the keep-everything plan runs the same layers unfused)
    _case("block2_gray_dst_full", _unet(16, 2, 4, output_stride=2), _single(3, 2), 2, (28, 44), 61, must=[("kv", L.KV_F16_BLOCK), ("kv", L.KV_STEM), ("kv", L.KV_FUSED)]),  # 14 x 22 behind the stem: the 8 x 32 tile cut both ways
    _case("block2_rgb_no_dst_full", _unet(16, 2, 4, output_stride=4, in_ch=3), _single(3, 4), 1, (26, 70), 62, must=[("kv", L.KV_F16_BLOCK), ("kv", L.KV_STEM)]),  # 13 x 35 behind the stem (the pool's zero padding, three tile columns); nobody reads the block's full-resolution output
    # (block_fuse 0 in the stem's own cases: their 16 -> 32 -> 32 middle block would run on block2_c32_f16_kernel, and a 32-channel tensor behind an unstored one differs from
    # the emulation's value in 0.8 - 0.9 % of its elements, on the stand-in as on the device -- too close to the 1 % cap to say anything about the stem)
    _case("stem_float_frames", _unet(16, 2, 2), _single(2, 1), 2, (12, 40), 63, {"block_fuse": 0}, float_frames=True, must=[("kv", L.KV_STEM)]),
    _case("stem_rgb_fp32_first_conv", _unet(16, 2, 2, in_ch=3), _single(2, 1), 1, (10, 36), 64, {"stem_f16mfma": 0, "block_fuse": 0}, must=[("kv", L.KV_STEM)]),
    _case("stem_gray_fp32_first_conv", _unet(16, 2, 2), _single(2, 1), 1, (10, 36), 65, {"stem_f16mfma": 0, "block_fuse": 0}, must=[("kv", L.KV_STEM)]),
    # ---- standalone heads (with and without the sigmoid), standalone bilinear in both arithmetics (keep-everything plans), transposed-conv decoder
    _case("heads_standalone_sigmoid", _unet(64, 1, 4), _multiclass(5, 1), 2, (20, 24), 71, {"head_fuse": 0}, must=[("kv", L.KV_F16_ROWS)]),
    _case("upsample_fp32math_standalone", _unet(24, 1.5, 4), _single(2, 1), 1, (20, 28), 72, {"upsample_f16math": 0}, must=[("kv", L.KV_F16)]),
    _case("transposed_conv_decoder", _unet(16, 2, 4, up_interpolate=False), _single(3, 1), 2, (20, 28), 73, must=[("kv", L.KV_F16)]),
]

# what the front end cannot reach, with the reason (test_the_table_reaches_every_form reads this)
UNREACHED = {
    "pool2x2_fmt_kernel": "every 2x2 pool of a UNet program follows a conv + ReLU, and Model._fuse_pools hands it to that conv (dst2): no OP_POOL is left in an inference "
                          "program, and the unfused (training) program runs exact fp32.  The kernel serves the ConvNeXt / Swin fp16 programs, which have their own emulations.",
}

# per case, from an MI355X (ROCm 7 hipcc, gfx950): (worst |d - r| / e where e > 0, worst share of d != r over the case's fp16 tensors); floor = 4 x the share, capped
MEASURED = {
    "persist_narrow_ragged": (1.000, 3.399e-04),
    "persist_odd_pool": (1.000, 6.614e-04),
    "persist_cin16_cin48": (1.000, 5.787e-04),
    "persist_two_n_tiles_64_128": (1.000, 7.378e-04),
    "persist_heads_17_32": (1.000, 4.232e-04),
    "persist_head_33_standalone": (1.000, 5.054e-04),
    "persist_pool_only_store": (1.000, 5.890e-04),
    "rows_a_mt3_mg4": (1.000, 7.813e-04),
    "rows_a_mt4_mg4": (1.000, 4.639e-04),
    "rows_a_mt5_mg4": (1.000, 3.906e-04),
    "rows_a_mt6_mg4": (1.000, 6.836e-04),
    "rows_a_mt7_mg4": (1.000, 8.240e-04),
    "rows_a_mt8_mg4": (1.000, 5.859e-04),
    "rows_a_mt9_mg4": (1.000, 7.161e-04),
    "rows_a_mt3_mg2": (1.000, 7.568e-04),
    "rows_a_mt4_mg2": (1.000, 5.859e-04),
    "rows_a_mt5_mg2": (0.500, 8.545e-04),
    "rows_a_mt6_mg2": (1.000, 9.766e-04),
    "rows_a_mt7_mg2": (1.000, 9.766e-04),
    "rows_a_mt8_mg2": (1.000, 7.568e-04),
    "rows_a_mt9_mg2": (1.000, 6.104e-04),
    "rows_u_mt3_mg4": (1.000, 4.735e-04),
    "rows_u_mt4_mg4": (1.000, 6.010e-04),
    "rows_u_mt5_mg4": (1.000, 5.682e-04),
    "rows_u_mt3_mg2": (1.000, 5.682e-04),
    "rows_u_mt4_mg2": (1.000, 1.202e-03),
    "rows_u_mt5_mg2": (1.000, 6.806e-04),
    "rows_lowres_f16math": (1.000, 1.302e-03),
    "rows_lowres_fp32math": (1.000, 5.208e-04),
    "rows_pool_only_store": (1.000, 6.200e-04),
    "rows_many_tiles": (1.000, 4.222e-04),
    "block2_gray_dst_full": (1.000, 1.573e-03),
    "block2_rgb_no_dst_full": (1.000, 4.464e-03),
    "stem_float_frames": (1.000, 5.859e-04),
    "stem_rgb_fp32_first_conv": (1.000, 6.944e-04),
    "stem_gray_fp32_first_conv": (1.000, 5.208e-04),
    "heads_standalone_sigmoid": (1.000, 5.208e-04),
    "upsample_fp32math_standalone": (1.000, 1.190e-03),
    "transposed_conv_decoder": (1.000, 3.962e-03),
}
for _c in CASES:
    _c.measured = MEASURED.get(_c.name)
    _c.floor = min(4.0 * _c.measured[1], SHARE_CAP) if _c.measured else None
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)

# the instantiations launch_conv3x3_f16_rows builds (f16_rows_kernels.hip: PH_ROWS_CASE 3 .. 9 for Wt % 16 == 0, PH_ROWS_CASE_U 3 .. 5 otherwise, each for MG 4 and 2)
ROWS_BUILT = {(True, mt, mg) for mt in range(3, 10) for mg in (4, 2)} | {(False, mt, mg) for mt in (3, 4, 5) for mg in (4, 2)}

_INPUTS = {}


def inputs(case):
    """(state dict, frames) of a case, built once.  Biases are drawn away from zero so that a bias added in the wrong place shows."""
    if case.name not in _INPUTS:
        g = torch.Generator().manual_seed(case.seed)
        sd = O.init_state(case.bb, case.heads, case.model_type, seed=case.seed, head_scale=1.0)
        for k in sd:
            if k.endswith(".bias"):
                sd[k] = (torch.rand(sd[k].shape, generator=g) - 0.5) * 0.2
        img = torch.randint(0, 256, (case.batch, case.bb["in_channels"], case.hw[0], case.hw[1]), dtype=torch.uint8, generator=g)
        if case.float_frames:
            img = img.float() / 255.0
        _INPUTS[case.name] = (sd, img)
    return _INPUTS[case.name]


def model(case):
    from sleap_nn_amd.architectures.model import Model

    sd, _img = inputs(case)
    m = Model("unet", case.bb, case.heads, case.model_type)
    m.load_state_dict(sd)
    return m


def emulation_kwargs(case):
    return {"upsample_f16math": int(case.options.get("upsample_f16math", 1)), "stem_f16mfma": int(case.options.get("stem_f16mfma", 1))}
