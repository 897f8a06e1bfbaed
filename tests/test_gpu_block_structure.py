"""Routing and kernels at block shapes other than two convs per block, against the oracle (pinned over the config grid by tests/test_host_cpu.py).

convs_per_block = 3: the first block is INPUT_CONV, CONV, CONV + pool (not the fused two-conv stem), every encoder level is a three-conv chain, the middle block has two
expand convs, and with 16 filters at rate 2 the pair (16 -> 32), (32 -> 32) that opens the second encoder block meets block2_c32_f16_kernel's conditions with NO pool behind
its second conv.  convs_per_block = 1 (no middle block, rate 1: the only one-conv UNet the reference runs): an INPUT_CONV directly in front of a POOL, which neither
plan-level fusion takes.  The reference's decoder blocks hold two refine convs in both (unet.py:203-216).

Bars are the project's own: heads within 1e-4 absolute and 1e-5 of their scale in exact fp32 (test_gpu_parity.py), split as close as exact (within 2x), plain fp16 within the
reference's 5e-3 of the oracle and within 3e-3 of the head's scale of the run with every fp16 fusion off (test_gpu_f16_pipe.py).  Every forward is run twice and must repeat
bit for bit.  All maps are far below one round of the persistent grids (at most 3 frames of 40 x 56 pixels where block2_c32_f16_kernel runs)."""
import itertools

import pytest
import torch

from oracle import cpu_ref as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CMS_ATOL = 1e-4
HEAD_RTOL = 1e-5
FP16_ATOL = 5e-3  # the reference's own fp16 bar (tests/inference/test_cuda.py:54-55)

# filters 16, max_stride 16, bottom-up heads (confmaps at output_stride, PAFs at twice that).  Frame sizes: 40 x 56 / 24 x 88 maps at stride 2 cut the 8 x 32 tiles of the
# block and stem kernels and the 16-pixel M tiles; batch 1 and 3; gray and RGB.  The decoder's concats need frames that are multiples of max_stride, so the ODD frame -- the
# pool's zero padding right behind a one-conv block -- runs on a network without a decoder (max_stride = output_stride = 4, head on the deepest feature).
CASES = {
    "cpb3_os2": dict(cpb=3, os=2, in_ch=1, batch=3, hw=(80, 112)),
    "cpb3_os4_rgb": dict(cpb=3, os=4, in_ch=3, batch=1, hw=(48, 176)),
    "cpb1_os2_rgb": dict(cpb=1, os=2, in_ch=3, batch=3, hw=(64, 144)),
    "cpb1_os4": dict(cpb=1, os=4, in_ch=1, batch=1, hw=(112, 80)),
    "cpb1_odd_no_decoder": dict(cpb=1, os=4, in_ch=1, batch=2, hw=(37, 45), max_stride=4),
}
ENC0_CONV1 = "backbone.encoders.0.encoder_stack.0.blocks.stack0_enc0_conv1"
ENC0_CONV2 = "backbone.encoders.0.encoder_stack.0.blocks.stack0_enc0_conv2"
ENC1_CONV0 = "backbone.encoders.0.encoder_stack.1.blocks.stack0_enc1_conv0"
ENC1_CONV1 = "backbone.encoders.0.encoder_stack.1.blocks.stack0_enc1_conv1"
ENC1_CONV2 = "backbone.encoders.0.encoder_stack.1.blocks.stack0_enc1_conv2"
_SETUP = {}


def _net(cpb, os, in_ch, max_stride=16, nodes=4):
    bb = {"in_channels": in_ch, "kernel_size": 3, "filters": 16, "filters_rate": 2 if cpb == 3 else 1, "max_stride": max_stride, "stem_stride": None,
          "middle_block": cpb == 3, "up_interpolate": True, "stacks": 1, "convs_per_block": cpb, "output_stride": os}
    names = [f"n{i}" for i in range(nodes)]
    if max_stride == os:  # no decoder: one head on the deepest feature
        return bb, {"confmaps": {"part_names": names, "output_stride": os}}, "single_instance"
    heads = {"confmaps": {"part_names": names, "output_stride": os}, "pafs": {"edges": [[names[i], names[i + 1]] for i in range(nodes - 1)], "output_stride": 2 * os}}
    return bb, heads, "bottomup"


def _setup(case):
    if case not in _SETUP:
        c = CASES[case]
        bb, heads, mt = _net(c["cpb"], c["os"], c["in_ch"], c.get("max_stride", 16))
        seed = sum(map(ord, case))
        sd = O.init_state(bb, heads, mt, seed=seed, head_scale=1.0)
        g = torch.Generator().manual_seed(seed)
        for k in sd:  # the oracle's biases are zero: give every conv one
            if k.endswith(".bias"):
                sd[k] = (torch.rand(sd[k].shape, generator=g) - 0.5) * 0.2
        img = torch.randint(0, 256, (c["batch"], c["in_ch"], c["hw"][0], c["hw"][1]), dtype=torch.uint8, generator=g)
        _SETUP[case] = (bb, heads, mt, sd, img, O.model_forward(sd, bb, heads, mt, img))
    return _SETUP[case]


def _run(sd, bb, heads, mt, img, precision="exact", opts=None, fused=True, reuse=None):
    """One model, two forwards that must give the same bits (as _run of test_gpu_f16_pipe.py) -> (outputs, kernel per op, model)."""
    from sleap_nn_amd.architectures.model import Model

    m = Model("unet", bb, heads, mt)
    m.load_state_dict(sd)
    m.to(DEV).set_precision(precision)
    if not fused:
        m.set_fusion(False)
    if reuse is not None:
        m.set_option("workspace_reuse", reuse)
    for k, v in (opts or {}).items():
        m.set_option(k, v)
    out = {k: v.cpu().clone() for k, v in m(img.to(DEV)).items()}
    again = {k: v.cpu() for k, v in m(img.to(DEV)).items()}
    for k in out:
        assert torch.equal(out[k], again[k]), (k, "not repeatable")
        assert torch.isfinite(out[k]).all(), k
    return out, m.last_kernels(), m


def _err(got, ref):
    return (got - ref).abs().max().item()


def _head_close(got, ref, key=None):
    err, scale = _err(got, ref), ref.abs().max().item()
    assert err <= CMS_ATOL, (key, err, scale)
    assert err <= HEAD_RTOL * scale, (key, err, scale)
    return err


def _op_index(m, label):
    hits = [i for i, o in enumerate(m.ops) if o.label.split("+")[0] == label]
    assert len(hits) == 1, (label, [o.label for o in m.ops])
    return hits[0]


def _assert_plan_shape(m, kv, cpb):
    """What the plan-level fusions must have made of the first block, and that the decoder has two refine convs per block."""
    from sleap_nn_amd import _lib as L

    assert m.ops[0].kind == L.OP_INPUT_CONV and m.ops[0].kind != L.OP_STEM, m.ops[0]
    assert L.KV_STEM not in kv, kv
    assert not any(o.kind == L.OP_STEM for o in m.ops)
    if cpb == 1 and m.ops is m.fused_ops:
        assert m.ops[1].kind == L.OP_POOL and m.ops[1].src0 == m.ops[0].dst  # the first conv's pool stays a launch of its own
    refine = [o.label for o in m.unfused_ops if "_refine_conv" in o.label]
    n_dec = sum(1 for o in m.unfused_ops if o.kind in (L.OP_UPSAMPLE, L.OP_CONVT))
    assert len(refine) == 2 * n_dec == 2 * len({l.split("_refine_conv")[0] for l in refine}) and not any(l.endswith("_refine_conv2") for l in refine), refine


@pytest.mark.parametrize("case", list(CASES))
def test_exact_and_split_forward_fused_and_unfused_programs_and_both_workspace_plans(case):
    """Exact fp32: the fused inference program and the op-by-op program, each with one memory range per slot and with shared slots -- heads within the parity bar of the
    oracle, the two programs within the same bar of each other, the two workspace plans of a program bit-identical (the same routing pins as
    test_workspace_reuse_shrinks_the_footprint_and_changes_no_bit), no fused stem in the plan and no stem kernel among the launches.  Split: the same absolute bar and an
    error within 2x of the exact path's (as test_split_precision_is_fp32_equivalent_on_the_benched_network)."""
    bb, heads, mt, sd, img, ref = _setup(case)
    cpb = CASES[case]["cpb"]
    pin = {"conv_splitk": 0, "conv_n32_wino2d": 0}  # inference-plan routes with their own rounding: off, so that both workspace plans run the same kernels
    outs = {}
    for fused, reuse in itertools.product((True, False), (1, 0)):
        outs[(fused, reuse)], kv, m = _run(sd, bb, heads, mt, img, "exact", pin, fused=fused, reuse=reuse)
        assert m.get_option("workspace_reuse") == float(reuse) and (m.ops is m.fused_ops) == fused
        _assert_plan_shape(m, kv, cpb)
    errs = {"exact": {}, "split": {}}
    for k, v in ref.items():
        for key, o in outs.items():
            e = _head_close(o[k], v, (case, key, k))
            errs["exact"][k] = max(errs["exact"].get(k, 0.0), e)
        _head_close(outs[(True, 1)][k], outs[(False, 0)][k], (case, "fused vs unfused", k))
        for fused in (True, False):
            assert torch.equal(outs[(fused, 1)][k], outs[(fused, 0)][k]), (case, fused, k)
    default, kv, m = _run(sd, bb, heads, mt, img, "exact")  # the default routing (what a user gets)
    _assert_plan_shape(m, kv, cpb)
    split, kv, m = _run(sd, bb, heads, mt, img, "split")
    assert m.get_option("conv_precision") == 1.0
    _assert_plan_shape(m, kv, cpb)
    for k, v in ref.items():
        errs["exact"][k] = max(errs["exact"][k], _head_close(default[k], v, (case, "default", k)))
        scale = v.abs().max().item()
        errs["split"][k] = _err(split[k], v)
        assert errs["split"][k] <= CMS_ATOL, (case, k, errs)
        assert errs["split"][k] / scale <= max(2.0 * _err(default[k], v) / scale, 2e-6), (case, k, errs, scale)
    print(f"block structure {case}: max |error| vs oracle exact {errs['exact']} split {errs['split']} (head scales { {k: round(v.abs().max().item(), 3) for k, v in ref.items()} })")


@pytest.mark.parametrize("case", list(CASES))
def test_fp16_forward_with_every_fusion_on_and_off_and_what_the_router_did(case):
    """Plain fp16: block_fuse x stem_f16mfma in {0, 1}^2 with conv_f16_rows 0 and 2 -- every combination within the reference's fp16 bar of the oracle and within
    3e-3 of the head's scale of the all-off run (the bar of test_fused_encoder_block_and_fp16_stem_against_the_unfused_kernels_and_the_oracle: the fused forms sum the taps in
    another order, which can flip an fp16 rounding of an activation).

    Three convs per block: with block_fuse = 1 the router DOES fuse the pair enc1_conv0 (16 -> 32), enc1_conv1 (32 -> 32) -- KV_F16_BLOCK on the first, KV_FUSED on the second
    -- although no pool follows the second conv (dst_pool = nullptr: the no-pool form of block2_c32_f16_kernel; its full-resolution tensor is compared on its own in
    test_no_pool_form_of_the_fused_encoder_block_tensor_itself); the third conv (+ pool) is a launch of its own.  The router's conditions are on padded channel counts, so it
    also takes the second and third conv of the FIRST block, (16 -> 16), (16 -> 16) + pool at full resolution, a pair that two-conv networks hand to the stem kernel: two
    KV_F16_BLOCK launches per forward, asserted by name.  One conv per block: nothing for the block kernel or the
    stem kernels to take, whatever the options say."""
    from sleap_nn_amd import _lib as L

    bb, heads, mt, sd, img, ref = _setup(case)
    cpb = CASES[case]["cpb"]
    outs, worst = {}, {}
    for rows, blk, stem in itertools.product((0, 2), (0, 1), (0, 1)):
        outs[(rows, blk, stem)], kv, m = _run(sd, bb, heads, mt, img, "fp16", {"conv_f16_rows": rows, "block_fuse": blk, "stem_f16mfma": stem})
        assert m.get_option("conv_precision") == 2.0
        _assert_plan_shape(m, kv, cpb)
        if cpb == 3:
            i = _op_index(m, ENC1_CONV0)
            assert m.ops[i].cin0 == 16 and m.ops[i].cout == 32 and m.ops[i + 1].label == ENC1_CONV1 and m.ops[i + 1].dst2 < 0  # no pool behind the pair's second conv
            assert m.ops[i + 2].label.split("+")[0] == ENC1_CONV2 and m.ops[i + 2].dst2 >= 0
            j = _op_index(m, ENC0_CONV1)
            assert j == 1 and m.ops[j].cin0 == m.ops[j].cout == 16 and m.ops[j + 1].label == ENC0_CONV2 + "+pool" and m.ops[j + 1].dst2 >= 0
            if blk:
                assert kv[i] == L.KV_F16_BLOCK and kv[i + 1] == L.KV_FUSED, (case, kv)
                assert kv[i + 2] not in (L.KV_FUSED, L.KV_F16_BLOCK, L.KV_NONE), (case, kv)
                assert kv[j] == L.KV_F16_BLOCK and kv[j + 1] == L.KV_FUSED and kv.count(L.KV_F16_BLOCK) == 2, (case, kv)  # enc0's pair as well, and nothing else
            else:
                assert L.KV_F16_BLOCK not in kv and kv[i + 1] != L.KV_FUSED, (case, kv)
            if (rows, blk, stem) == (0, 1, 1):
                print(f"block structure {case} fp16 kernels per op (defaults but conv_f16_rows = 0):", [(o.label.split(".")[-1], L.KV_NAMES[c].split(" ")[0]) for o, c in zip(m.ops, kv)])
        else:
            assert L.KV_F16_BLOCK not in kv and L.KV_STEM not in kv, (case, kv)
        for k, v in ref.items():
            e = _err(outs[(rows, blk, stem)][k], v)
            worst[k] = max(worst.get(k, 0.0), e)
            assert e <= FP16_ATOL, (case, rows, blk, stem, k, e)
    for k, v in ref.items():
        scale = max(v.abs().max().item(), 1.0)
        for key, o in outs.items():
            assert _err(o[k], outs[(0, 0, 0)][k]) <= 3e-3 * scale, (case, key, k)
    default, kv, m = _run(sd, bb, heads, mt, img, "fp16")
    _assert_plan_shape(m, kv, cpb)
    assert (L.KV_F16_BLOCK in kv) == (cpb == 3)
    if cpb == 3:
        print(f"block structure {case} fp16 kernels per op (default options):", [(o.label.split(".")[-1], L.KV_NAMES[c].split(" ")[0]) for o, c in zip(m.ops, kv)])
    for k, v in ref.items():
        worst[k] = max(worst[k], _err(default[k], v))
        assert _err(default[k], v) <= FP16_ATOL, (case, "default", k)
    print(f"block structure {case}: max |error| vs oracle fp16 {worst}")


@pytest.mark.parametrize("batch,hw", [(3, (80, 112)), (1, (48, 176))])
def test_no_pool_form_of_the_fused_encoder_block_tensor_itself(batch, hw):
    """block2_c32_f16_kernel without a pool behind its second conv (three convs per block: the pair enc1_conv0, enc1_conv1) -- the full-resolution tensor ITSELF against the
    two separate launches (block_fuse = 0) and against the oracle's activation.  Keep-everything plans do not fuse (the router asks for an inference plan), so the tensor is
    carried to a head on its stride by weights that copy it: enc1_conv2, the skip half of the stride-2 decoder block's first refine conv, its second refine conv and a
    32-channel confidence-map head are all set to the identity (centre tap 1 on the diagonal, zero bias; the tensor is >= 0 behind its ReLU, products by 1 and sums with 0
    are exact in fp16 and fp32).  The oracle confirms the construction: its head output IS its enc1_conv1 activation."""
    from sleap_nn_amd import _lib as L

    bb, heads, mt = _net(3, 2, 1, nodes=32)
    heads["pafs"]["edges"] = heads["pafs"]["edges"][:3]
    sd = O.init_state(bb, heads, mt, seed=hw[1], head_scale=1.0)
    g = torch.Generator().manual_seed(hw[0])
    for k in sd:
        if k.endswith(".bias"):
            sd[k] = (torch.rand(sd[k].shape, generator=g) - 0.5) * 0.2
    sd[ENC1_CONV1 + ".weight"] = sd[ENC1_CONV1 + ".weight"] * 4.0  # the tensor at O(1), where the absolute fp16 bars below are a fraction of a percent of it
    dec = "backbone.decoders.0.decoder_stack.2.blocks.stack0_dec2_s4_to_s2_refine_conv"
    eye = torch.zeros((32, 32, 3, 3))
    eye[torch.arange(32), torch.arange(32), 1, 1] = 1.0
    for name in (ENC1_CONV2, dec + "1"):
        assert sd[name + ".weight"].shape == eye.shape
        sd[name + ".weight"], sd[name + ".bias"] = eye.clone(), torch.zeros(32)
    assert sd[dec + "0.weight"].shape == (32, 32 + 64, 3, 3)  # concat (skip, up-sampled): the skip comes first
    sd[dec + "0.weight"], sd[dec + "0.bias"] = torch.cat([eye, torch.zeros((32, 64, 3, 3))], dim=1), torch.zeros(32)
    head = "head_layers.0.MultiInstanceConfmapsHead.0"
    assert sd[head + ".weight"].shape == (32, 32, 1, 1)
    sd[head + ".weight"], sd[head + ".bias"] = torch.eye(32).reshape(32, 32, 1, 1).clone(), torch.zeros(32)
    img = torch.randint(0, 256, (batch, 1, hw[0], hw[1]), dtype=torch.uint8, generator=g)
    acts = {}
    ref = O.model_forward(sd, bb, heads, mt, img, collect=acts)
    tensor = acts[ENC1_CONV1]
    assert torch.equal(ref["MultiInstanceConfmapsHead"], tensor) and tensor.shape[-2:] == (hw[0] // 2, hw[1] // 2)
    scale = tensor.abs().max().item()
    assert scale > 0.5 and (tensor > 0).float().mean().item() > 0.2  # a live tensor (far above the fp16 bars below), not a field of zeros
    exact, kv, m = _run(sd, bb, heads, mt, img, "exact")
    assert _err(exact["MultiInstanceConfmapsHead"], tensor) <= CMS_ATOL  # the carrier copies the tensor on the device as well
    got = {}
    for blk in (1, 0):
        out, kv, m = _run(sd, bb, heads, mt, img, "fp16", {"block_fuse": blk})
        i = _op_index(m, ENC1_CONV0)
        assert m.ops[i + 1].label == ENC1_CONV1 and m.ops[i + 1].dst2 < 0
        assert (kv[i] == L.KV_F16_BLOCK and kv[i + 1] == L.KV_FUSED) if blk else (L.KV_F16_BLOCK not in kv), (blk, kv)
        got[blk] = out["MultiInstanceConfmapsHead"]
        assert _err(got[blk], tensor) <= FP16_ATOL * max(1.0, scale), (blk, _err(got[blk], tensor), scale)  # the fp16 bar of the goldens' activations
        assert _err(out["PartAffinityFieldsHead"], ref["PartAffinityFieldsHead"]) <= FP16_ATOL
    assert _err(got[1], got[0]) <= 3e-3 * max(scale, 1.0), (_err(got[1], got[0]), scale)
    # the tensor's image border and the cut tiles on their own: the last row / column and the columns behind the last whole 32-pixel tile
    h, w = tensor.shape[-2:]
    for region in (got[1][..., h - 1, :], got[1][..., :, w - 1], got[1][..., :, (w // 32) * 32:]):
        assert region.abs().max().item() > 0
    print(f"no-pool block2 tensor {tuple(tensor.shape)}: scale {scale:.3f}, fused vs oracle {_err(got[1], tensor):.2e}, unfused vs oracle {_err(got[0], tensor):.2e}, "
          f"fused vs unfused {_err(got[1], got[0]):.2e}")
