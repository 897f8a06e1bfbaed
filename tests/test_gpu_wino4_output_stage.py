"""conv3x3_wino4_kernel's output stage stores 16 bytes per lane: a thread still computes the 4 x 4 outputs of one channel PAIR, then the two lanes of a channel quad trade half of
every output row through DPP, so that the even lane holds the whole quad of columns 0, 1 and the odd lane of columns 2, 3.  A wrong select mask, lane pairing, pixel offset of the
odd lane, pool column or ReLU-mask address shows as swapped channel pairs or columns of single pixels, in every tile -- or only where `live` cuts tiles and dead channel quads, if the
exchange were to depend on the lanes that store.  So: every channel count that changes the N-tile layout (one, two, three N tiles; 16 and 48 channels mod 64), maps that cut tiles
and maps of several workgroup tiles, every variant of the stage (pool with and without the full-resolution store, folded bilinear, split K, the backward's ReLU mask).

Small networks through ``Model`` with ``conv_wino4 = 3`` (the kernel wherever the shape fits), as tests/test_gpu_wino4_raw_slot.py builds them."""
import ctypes as C

import pytest
import torch

from oracle import cpu_ref as O
from tests.test_gpu_parity import W4_RTOL  # the F(4x4,3x3) layers' bar against the oracle, of the head's scale: stated once, there

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
KERNELS_RTOL = 3e-5  # against the same network with conv_wino4 = 0, of the head's scale: the bar tests/test_gpu_wino4_raw_slot.py holds the two kernel families to

# 20 x 36: multiples of 4, not of 16 / 32: the second row and column of workgroup tiles are cut, `live` masks whole Winograd tiles.  36 x 68: 3 x 3 workgroup tiles.
SIZES = {"20x36": (20, 36), "36x68": (36, 68)}

VARIANTS = {
    # decoder down to stride 2 only: nobody reads the full-resolution output of the first level's conv + pool (pool alone is stored: skip_dst), the second level's
    # (128 channels at 20 x 36) is a skip connection (both tensors stored); the decoder conv reads 128 + 256 channels, the 256 from the 10 x 18 map through the folded bilinear
    "pool_with_and_without_dst": dict(filters=64, rate=2, max_stride=4, output_stride=2, hw=(40, 72), options={"workspace_reuse": 1}, min_wino4=5, pooled=2),
    # K split in three on every layer from 128 input channels: the plain instantiation (128 -> 128, with the second stage's pool) and the folded-bilinear one (128 + 128 -> 128)
    "forced_split_k": dict(filters=128, rate=1, max_stride=2, output_stride=1, hw=(20, 36), options={"conv_splitk": 3}, min_wino4=3, split=(3, 20, 36, 256, 128, 3)),
    # 72 / 108 / 162 channels, padded to 80 / 112 / 176: the last N tile holds 16 or 48 channels: whole channel quads of a round are dead, and the 16-channel tile keeps the
    # channel order of a half-empty tile while the 48-channel one has the full-line order
    "dead_channel_quads": dict(filters=72, rate=1.5, max_stride=4, output_stride=1, hw=(40, 72), options={}, min_wino4=7),
}


def _bb(filters, rate, max_stride, output_stride):
    return {"in_channels": 1, "kernel_size": 3, "filters": filters, "filters_rate": rate, "max_stride": max_stride, "stem_stride": None,
            "middle_block": True, "up_interpolate": True, "stacks": 1, "convs_per_block": 2, "output_stride": output_stride}


def _check(name, bb, hw, options, min_wino4, pooled=0):
    """Batch 3 on the kernel against the oracle and against the other kernels; frame 0 of the batch bitwise against frame 0 alone."""
    from sleap_nn_amd import _lib as L
    from sleap_nn_amd.architectures.model import Model

    heads = {"confmaps": {"part_names": ["a", "b", "c"], "output_stride": bb["output_stride"]}}
    sd = O.init_state(bb, heads, "single_instance", seed=hw[0] + bb["filters"], head_scale=1.0)
    img = torch.randint(0, 256, (3, 1) + hw, dtype=torch.uint8, generator=torch.Generator().manual_seed(hw[1]))
    ref = O.model_forward(sd, bb, heads, "single_instance", img)["SingleInstanceConfmapsHead"]
    outs = {}
    for run, w4, frames in (("wino4", 3, img), ("alone", 3, img[:1]), ("other", 0, img)):
        m = Model("unet", bb, heads, "single_instance")
        m.load_state_dict(sd)
        m.set_option("conv_wino4", w4).set_option("conv_smallmap", 0)
        for k, v in options.items():
            m.set_option(k, v)
        m.to(DEV)
        outs[run] = m(frames.to(DEV).contiguous())["SingleInstanceConfmapsHead"].cpu()
        kv = m.last_kernels()
        n4 = sum(1 for k in kv if k == L.KV_WINO4)
        if w4:
            assert n4 >= min_wino4, (n4, [L.KV_NAMES.get(k, k) for k in kv])
            ups = [i for i, op in enumerate(m.ops) if op.kind == L.OP_UPSAMPLE]
            assert ups and all(kv[i + 1] == L.KV_WINO4 for i in ups), "every decoder's bilinear x2 must ride in the F(4x4,3x3) kernel"
            assert sum(1 for op, k in zip(m.ops, kv) if op.kind == L.OP_CONV and op.dst2 >= 0 and k == L.KV_WINO4) >= max(pooled, 1), "a conv + pool launch must run on the kernel"
        else:
            assert n4 == 0
    scale = ref.abs().max().item()
    err_ref = (outs["wino4"] - ref).abs().max().item()
    err_other = (outs["wino4"] - outs["other"]).abs().max().item()
    print(f"{name}: scale {scale:.4g}, vs oracle {err_ref / scale:.3g} of scale, vs the other kernels {err_other / outs['other'].abs().max().item():.3g}")
    assert err_ref <= W4_RTOL * scale, (err_ref, scale)
    assert err_other <= KERNELS_RTOL * outs["other"].abs().max().item(), (err_other, scale)
    assert torch.equal(outs["wino4"][:1], outs["alone"]), "frame 0 of a batch of 3 must not depend on the batch"


@pytest.mark.parametrize("size", sorted(SIZES))
@pytest.mark.parametrize("channels", [64, 128, 192])
def test_every_channel_quad_lands_on_its_pixel(channels, size):
    """One, two and three N tiles of 64 channels (a lane pair's quad index runs over both N halves and both rounds); the encoder's conv + pool and the folded-bilinear decoder
    conv (2 x channels in) on the kernel (the 64-channel net's last conv carries the head and runs elsewhere).  No K split (its slice count follows the batch: frame 0 would be
    summed in another order)."""
    _check(f"{channels} channels at {size}", _bb(channels, 1, 2, 1), SIZES[size], {"conv_splitk": 0}, 2)


@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_output_stage_variants(variant):
    from sleap_nn_amd import _lib as L

    v = VARIANTS[variant]
    if "split" in v:  # the layer this case is there for does take the split on this kernel (the host's plan, asked directly)
        out = (C.c_int64 * 4)()
        assert L.lib().ph_debug_split_plan(*v["split"], 256, out) == 0 and out[1] == 3, list(out)
    _check(variant, _bb(v["filters"], v["rate"], v["max_stride"], v["output_stride"]), v["hw"], v["options"], v["min_wino4"], v.get("pooled", 0))


def test_backward_relu_mask_rides_in_the_16_byte_stores():
    """A data-gradient conv on the kernel that completes the gradient of a conv + ReLU output applies that ReLU's mask in its stores (ConvArgs::relu_mask_src): the mask is now
    loaded 16 bytes wide for the pixels the lane stores, after the exchange.  64-channel UNet at 20 x 36 (2 x 2 workgroup tiles, the second row and column cut) through
    TrainingModule(wino4=True); every gradient against float64 at the floor tests/_backward_cases.py holds `dgrad_wino4_everywhere` to.  (Seed 79: the smallest |ReLU pre-activation|
    of the reference is 2.1e-6; at 36 x 68 no seed of the first hundred keeps every ReLU a rounding error away from its kink.)"""
    from sleap_nn_amd import _lib as L
    from tests import _backward_cases as T

    like = T.BY_NAME["dgrad_wino4_everywhere"]
    case = T.Case("output_stage_relu_mask", "unet", dict(like.bb), like.heads, like.model_type, 2, (20, 36), 79, dict(like.options), module_kw={"wino4": True}, floor=like.floor)
    assert T.relu_margin(case) >= 1e-6  # (no ReLU of the reference on its kink: tests/test_backward_routes_cpu.py)
    sd, img, targets, lw = T.inputs(case)
    tm = T.module(case, DEV)
    dev_t = {k: v.to(DEV) for k, v in targets.items()}
    tm.forward_backward(img.to(DEV), dev_t)
    torch.cuda.synchronize()
    words = [L.br_decode(w) for w in tm.model.last_backward_routes()]
    carried = [i for i, (op, w) in enumerate(zip(tm.model.ops, words)) if op.kind == L.OP_CONV and L.KV_WINO4 in w["dgrad"] and w["folded_mask"]]
    assert carried, words
    got = tm.named_grads()
    _l32, g32 = T.reference(case, False)
    _l64, g64 = T.reference(case, True)
    e_hip, e_ref = T.e_rel(got, g64), T.e_rel(g32, g64)
    worst = max(e_hip, key=e_hip.get)
    print(f"worst e_hip {e_hip[worst]:.3e} ({worst}, e_ref {e_ref[worst]:.2e}); floor {case.floor:.1e}; data-gradient convs with the mask on the kernel: ops {carried}")
    for k in g64:
        assert e_hip[k] <= max(case.floor, 2.0 * e_ref[k]), (k, e_hip[k], e_ref[k])
    tm.close()
