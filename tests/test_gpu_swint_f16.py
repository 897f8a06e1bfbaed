"""Swin inference on the fp16 matrix pipe (``set_precision("fp16", swint_f16=True)``; swin_f16_kernels.hip + the fp16 row GEMM / LayerNorm of
convnext_f16_kernels.hip) against tests/swin_ref.py.

Bar: ``FP16_ATOL`` = 5e-3, the project's bar for the fp16 precision (tests/test_gpu_convnext_f16.py), as max |got - ref| / max(1, max |ref|), on the heads and on
every labelled block (``read_activation``).  Shapes, images and seeds are those of tests/test_gpu_swint.py.  tools/swint_f16_emulation.py predicts 0.9 to 1.4e-3 at
the heads for the storage plan the device uses; every case prints the device's head error next to the emulation's and asserts the device stays within
``DEVICE_VS_EMULATION`` x 1.5 of it (the margin: accumulation-order differences flipping fp16 roundings).
"""
import functools
import hashlib
import importlib.util
import os

import pytest
import torch

from oracle import cpu_ref as O
from tests import swin_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FP16_ATOL = 5e-3
PLAN_ATOL = 2e-3  # inference plan vs keep-everything plan: a few fp16 ulps at the heads (tests/test_gpu_convnext_f16.py)
SMALL = {"embed": 32, "depths": [2, 2, 2, 2], "num_heads": [1, 2, 4, 8]}
# largest device head error / emulation head error over the cases below, measured on an MI355X (0.81 to 1.27; DESIGN.md 4.4c lists them per case)
DEVICE_VS_EMULATION = 1.27

_spec = importlib.util.spec_from_file_location("swint_f16_emulation", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "swint_f16_emulation.py"))
E = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(E)


def _bb(**kw):
    bb = {"model_type": None, "arch": SMALL, "in_channels": 1, "patch_size": 4, "window_size": 7, "kernel_size": 3, "filters_rate": 2, "convs_per_block": 2,
          "up_interpolate": True, "stem_patch_stride": 2, "output_stride": 2, "max_stride": 32, "pre_trained_weights": None}
    bb.update(kw)
    return bb


def _heads(n, stride=2):
    return {"confmaps": {"part_names": [str(i) for i in range(n)], "sigma": 2.5, "output_stride": stride}}


def _u8(shape, seed):
    return torch.randint(0, 256, shape, dtype=torch.uint8, generator=torch.Generator().manual_seed(seed))


def _reference(bb, heads, mt, sd, img):
    """(swin_ref heads, swin_ref labelled activations, head error of the emulation's form (a))."""
    collect = {}
    ref = R.model_forward(sd, bb, heads, mt, img, collect=collect)
    return ref, collect, E.head_error(E.forward(sd, bb, heads, mt, img, "f16"), ref)


@functools.lru_cache(maxsize=None)
def _case(name):
    """(bb, heads, model type, state dict, image, reference heads, reference activations, emulation head error) -- computed once, shared, never modified."""
    if name == "small":  # stage maps 32x48, 16x24, 8x12, 4x6 -> padded 35x49, 21x28, 14x14, 7x7; 2 * 5 * 7 windows x 1 head at stage 0: 70 waves, 17.5 workgroups
        bb, heads, mt, img, seed = _bb(), _heads(5), "single_instance", _u8((2, 1, 64, 96), 11), 7
    elif name == "mixed":  # last stage 4x12: pH = 7 turns the row shift off, pW = 14 keeps the column shift on
        bb, heads, mt, img, seed = _bb(), _heads(3), "single_instance", _u8((2, 1, 64, 192), 12), 8
    elif name in ("w4", "w8"):  # N = 16 (one tile, half of it dead) / N = 64 (two full tiles)
        w = int(name[1])
        bb, heads, mt, img, seed = _bb(window_size=w), _heads(3), "single_instance", _u8((1, 1, 64, 64), 14), 10 + w
    elif name == "tiny":  # 96 .. 768 channels over 3 / 6 / 12 / 24 heads, the 1536-channel merge norm, N tiles of three 32-channel blocks
        bb, heads, mt, seed = _bb(model_type="tiny", arch=None, in_channels=3), _heads(13), "centered_instance", 7
        img = torch.rand((1, 3, 64, 64), generator=torch.Generator().manual_seed(3))
    elif name == "batch4":
        bb, heads, mt, img, seed = _bb(), _heads(3), "single_instance", _u8((4, 1, 128, 128), 15), 21
    else:
        raise KeyError(name)
    sd = R.init_state_swint(bb, heads, mt, seed=seed)
    return (bb, heads, mt, sd, img) + _reference(bb, heads, mt, sd, img)


def _model(bb, heads, mt, sd, precision="fp16", keep=False, swint_f16=True):
    from sleap_nn_amd.architectures.model import Model

    m = Model("swint", bb, heads, mt)
    m.load_state_dict(sd, strict=True)
    m.to(DEV).set_keep_activations(keep)
    return m.set_precision(precision, swint_f16=swint_f16)


def _err(got, ref):
    return (got.cpu() - ref).abs().max().item() / max(1.0, ref.abs().max().item())


def _assert_f16_route(m):
    """Every op of the last forward ran an fp16 kernel: no fp32 attention, no fp32 row GEMM, no fp32 MLP kernel."""
    from sleap_nn_amd import _lib as L

    want = {L.OP_PATCH_STEM: {L.CNX_KV_F16_STEM}, L.OP_LAYERNORM: {L.CNX_KV_F16_LN}, L.OP_LINEAR: {L.CNX_KV_F16_GEMM}, L.OP_WINDOW_ATTN: {L.SWIN_KV_WINDOW_ATTN_F16},
            L.OP_PATCH_MERGE: {L.SWIN_KV_F16_MERGE_LN}, L.OP_CONV: {L.KV_F16, L.KV_F16_ROWS, L.KV_F16_BLOCK, L.KV_FUSED}}
    kv = list(m.last_kernels())
    assert m.get_option("conv_precision") == 2.0 and m.get_option("swint_f16") == 1.0
    for op, code in zip(m.ops, kv):
        if op.kind in want:
            assert code in want[op.kind], (op.label, op.kind, code)
    assert L.SWIN_KV_WINDOW_ATTN not in kv and L.KV_ROWGEMM not in kv and L.KV_MLP not in kv, kv
    return kv


def _check_heads(name, out, ref, emu):
    worst = 0.0
    for k, t in ref.items():
        assert out[k].shape == t.shape
        worst = max(worst, _err(out[k], t))
    print(f"{name}: device head error {worst:.3e}, emulation {emu:.3e}, ratio {worst / emu:.2f}")
    assert worst <= FP16_ATOL, (name, worst)
    assert worst <= 1.5 * DEVICE_VS_EMULATION * emu, (name, worst, emu)
    return worst


def _run(name, check_blocks=True):
    """Forward of case ``name`` on the fp16 route: heads (and, on the keep-activations plan, every labelled block) within the bar -> (model, device outputs)."""
    bb, heads, mt, sd, img, ref, collect, emu = _case(name)
    m = _model(bb, heads, mt, sd, keep=check_blocks)
    out = {k: v.clone() for k, v in m(img.to(DEV)).items()}
    torch.cuda.synchronize()
    _assert_f16_route(m)
    if check_blocks:
        worst, checked = {}, 0
        for lbl, t in collect.items():
            if lbl not in m.backbone.labels:
                continue
            worst[lbl] = _err(m.read_activation(lbl, t.shape[0], t.shape[-2:]), t)
            checked += 1
        top = max(worst, key=worst.get)
        print(f"{name}: worst block {top} {worst[top]:.3e}")
        bad = {k: v for k, v in worst.items() if not v <= FP16_ATOL}
        assert not bad, bad
        assert checked >= 4 * sum(R.arch_of(bb)["depths"]) // 2
    _check_heads(name, out, ref, emu)
    return m, out


def test_route_padding_both_axes_shift_and_single_window():
    """SMALL arch, window 7, 2 x 64 x 96 uint8: padding in both axes under a shift, a single-window stage, a workgroup count that is no multiple of four at the
    one-head stage.  Eight attention ops on the new code, nothing on the fp32 attention or row-GEMM code; blocks and heads within the bar; a second forward gives the same bits."""
    from sleap_nn_amd import _lib as L

    m, out = _run("small")
    kv = list(m.last_kernels())
    assert kv.count(L.SWIN_KV_WINDOW_ATTN_F16) == 8
    assert kv.count(L.SWIN_KV_F16_MERGE_LN) == 3
    img = _case("small")[4]
    again = m(img.to(DEV))
    for k in out:
        assert torch.equal(out[k], again[k]), (k, "not repeatable")


def test_mixed_shift_rows_off_columns_on():
    _run("mixed")


@pytest.mark.parametrize("window", [4, 8])
def test_window_4_and_8(window):
    _run(f"w{window}")


def test_padded_tokens_take_part_as_keys():
    """qkv.bias = +-3 in the two blocks whose map is padded in both axes (plain and shifted): a padded token's q, k, v are fp16(qkv.bias).  Within the bar, and
    far from the run with that bias zeroed."""
    bb, heads, mt = _bb(), _heads(3), "single_instance"
    g = torch.Generator().manual_seed(13)
    img = torch.randint(0, 256, (2, 1, 64, 96), dtype=torch.uint8, generator=g)
    sd = R.init_state_swint(bb, heads, mt, seed=9)
    outs = []
    for scale in (3.0, 0.0):
        for blk in ("backbone.enc.features.1.0", "backbone.enc.features.1.1"):
            key = blk + ".attn.qkv.bias"
            sd[key] = torch.sign(torch.randn(sd[key].shape, generator=g)) * scale
        ref, _collect, emu = _reference(bb, heads, mt, sd, img)
        m = _model(bb, heads, mt, sd)
        out = m(img.to(DEV))
        torch.cuda.synchronize()
        _assert_f16_route(m)
        _check_heads(f"qkv.bias +-{scale}", out, ref, emu)
        outs.append(out["SingleInstanceConfmapsHead"].cpu())
    assert (outs[0] - outs[1]).abs().max().item() > 20 * FP16_ATOL


def test_swin_tiny_centered_instance_rgb_float():
    _run("tiny", check_blocks=False)


def test_encoder_is_batch_invariant():
    """Batch 4 at 128 x 128 (400 windows at stage 0), keep-activations plan: frame 2's ``backbone.enc.norm`` activation equals the same frame run alone, bit for
    bit.  (The decoder's kernel choice may depend on the batch: the comparison stops at the encoder.)"""
    bb, heads, mt, sd, img, ref, _collect, emu = _case("batch4")
    m = _model(bb, heads, mt, sd, keep=True)
    out = {k: v.clone() for k, v in m(img.to(DEV)).items()}
    torch.cuda.synchronize()
    _assert_f16_route(m)
    _check_heads("batch4", out, ref, emu)
    hw = (128 // 2 // 8, 128 // 2 // 8)
    a4 = m.read_activation("backbone.enc.norm", 4, hw)[2:3].clone()
    m(img[2:3].to(DEV))
    a1 = m.read_activation("backbone.enc.norm", 1, hw)
    torch.cuda.synchronize()
    assert a4.shape == a1.shape and a4.abs().max().item() > 0
    assert torch.equal(a4, a1)


def test_inference_plan_agrees_with_the_keep_everything_plan():
    """workspace_reuse 1 vs the plan that keeps every tensor: a few fp16 ulps at the heads; the recycling plan passes the no-overlap / liveness invariant of
    tests/test_gpu_plan_hazards.py, and every residual GEMM was handed its block input as a source."""
    from sleap_nn_amd import _lib as L
    from tests.test_gpu_plan_hazards import _check_plan

    bb, heads, mt, sd, img, ref, _collect, emu = _case("small")
    keep = _model(bb, heads, mt, sd, keep=True)
    a = {k: v.clone() for k, v in keep(img.to(DEV)).items()}
    inf = _model(bb, heads, mt, sd, keep=False)
    b = inf(img.to(DEV))
    torch.cuda.synchronize()
    assert inf.get_option("workspace_reuse") == 1.0
    _assert_f16_route(inf)
    for k, t in ref.items():
        d = (a[k] - b[k]).abs().max().item() / max(1.0, t.abs().max().item())
        print(k, f"plans differ by {d:.2e}")
        assert d <= PLAN_ATOL, (k, d)
    _check_heads("small, inference plan", b, ref, emu)
    _check_plan(inf, "swint small fp16")
    rows = inf.last_ranges()
    residual_ops = [p for p, o in enumerate(inf.ops) if o.kind == L.OP_LINEAR and o.flags & L.FLAG_RESIDUAL]
    assert len(residual_ops) == 16
    for p in residual_ops:
        assert any(op == p and not is_dst and slot == inf.ops[p].src1 for op, _ln, is_dst, slot, _o, _n in rows), p


def test_weight_images_follow_live_parameters():
    """qkv, proj, reduction and bias-table values changed: after ``load_state_dict`` the fp16 forward matches the reference of the NEW weights, and a handle
    created from the old weights and re-bound to the new arena (ph_model_set_params) gives the bits of the fresh handle."""
    from sleap_nn_amd.architectures.model import Model

    bb, heads, mt, sd_a, img, ref_a, _collect, _emu = _case("small")
    g = torch.Generator().manual_seed(77)
    sd_b = {k: v.clone() for k, v in sd_a.items()}
    changed = [k for k in sd_b if k.endswith((".attn.qkv.weight", ".attn.qkv.bias", ".attn.proj.weight", ".reduction.weight", ".relative_position_bias_table"))]
    assert len(changed) == 8 * 4 + 3
    for k in changed:
        sd_b[k] = sd_b[k] + 0.3 * sd_b[k].abs().mean() * torch.randn(sd_b[k].shape, generator=g)
    ref_b, _c, emu_b = _reference(bb, heads, mt, sd_b, img)
    m = _model(bb, heads, mt, sd_a)
    from_a = {k: v.clone() for k, v in m(img.to(DEV)).items()}
    m.load_state_dict(sd_b, strict=True)
    want = {k: v.clone() for k, v in m(img.to(DEV)).items()}
    torch.cuda.synchronize()
    _assert_f16_route(m)
    _check_heads("new weights", want, ref_b, emu_b)
    donor = Model("swint", bb, heads, mt)
    donor.load_state_dict(sd_b, strict=True)
    live = _model(bb, heads, mt, sd_a)
    live.bind_live_params(donor.flat_params().to(DEV))
    got = live(img.to(DEV))
    torch.cuda.synchronize()
    _assert_f16_route(live)
    for k in want:
        assert torch.equal(got[k], want[k]), (k, (got[k] - want[k]).abs().max().item())
        assert not torch.equal(from_a[k], want[k]), k  # (the two weight sets do differ)


def test_switching_precisions_on_one_handle():
    """exact -> fp16 with swint_f16 -> exact: the last output is bitwise the first; ``set_precision("fp16", swint_f16=False)`` gives the exact output again."""
    from sleap_nn_amd import _lib as L

    bb, heads, mt, sd, img, ref, _collect, emu = _case("small")
    m = _model(bb, heads, mt, sd, precision="exact", swint_f16=None)
    x = img.to(DEV)
    first = {k: v.clone() for k, v in m(x).items()}
    assert L.SWIN_KV_WINDOW_ATTN in m.last_kernels()
    m.set_precision("fp16", swint_f16=True)
    half = {k: v.clone() for k, v in m(x).items()}
    _assert_f16_route(m)
    _check_heads("small, switched", half, ref, emu)
    m.set_precision("exact")
    last = {k: v.clone() for k, v in m(x).items()}
    assert L.SWIN_KV_WINDOW_ATTN in m.last_kernels()
    m.set_precision("fp16", swint_f16=False)
    off = {k: v.clone() for k, v in m(x).items()}
    kv = m.last_kernels()
    assert L.SWIN_KV_WINDOW_ATTN in kv and L.SWIN_KV_WINDOW_ATTN_F16 not in kv
    torch.cuda.synchronize()
    for k in first:
        assert torch.equal(last[k], first[k]), k
        assert torch.equal(off[k], first[k]), k
        assert not torch.equal(half[k], first[k]), k


# sha256 of the head output of the ConvNeXt forward below in the fp16 precision with convnext_f16 at the commit before the Swin fp16 route existed
CONVNEXT_F16_SHA256 = "13f2f04f1a0635752cab30ecc9c8e13f70ff48604b5fd32538f57d0f888fdb4b"


def test_programs_that_stay_exact():
    """The unfused (training-style) program, the split precision, the swint_f16 option without the fp16 precision, convnext_f16 on a Swin program and a Swin program
    with a class-vector head keep the exact path bit for bit; a ConvNeXt model's convnext_f16 output is what it was, with or without swint_f16."""
    from sleap_nn_amd import _lib as L
    from sleap_nn_amd.architectures.model import Model

    bb, heads, mt, sd, img, _ref, _collect, _emu = _case("small")
    x = img.to(DEV)

    def run(model):
        out = {k: v.clone() for k, v in model(x).items()}
        kv = list(model.last_kernels())
        assert L.SWIN_KV_WINDOW_ATTN in kv, kv
        assert not ({L.SWIN_KV_WINDOW_ATTN_F16, L.SWIN_KV_F16_MERGE_LN, L.CNX_KV_F16_STEM, L.CNX_KV_F16_LN, L.CNX_KV_F16_GEMM, L.KV_F16, L.KV_F16_ROWS} & set(kv)), kv
        return out

    exact = run(_model(bb, heads, mt, sd, precision="exact"))
    split = run(_model(bb, heads, mt, sd, precision="split"))
    other = run(_model(bb, heads, mt, sd, precision="fp16", swint_f16=None).set_option("convnext_f16", 1))  # (the ConvNeXt switch does not move a Swin program)
    for k in exact:
        assert torch.equal(split[k], exact[k]) and torch.equal(other[k], exact[k]), k
    # the op-by-op program a training handle runs (conv_precision 0 whatever is set; Model.train() itself refuses a swint backbone)
    tr_e = _model(bb, heads, mt, sd, precision="exact").set_fusion(False)
    tr_f = _model(bb, heads, mt, sd, precision="fp16").set_fusion(False)
    a, b = run(tr_e), run(tr_f)
    assert tr_f.get_option("conv_precision") == 0.0 and tr_f.get_option("swint_f16") == 1.0
    for k in a:
        assert torch.equal(a[k], b[k]), k
    # multi_class_topdown: confidence maps + a class-vector head on the middle feature
    hv = {"confmaps": {"part_names": ["a", "b", "c"], "anchor_part": None, "sigma": 2.5, "output_stride": 2},
          "class_vectors": {"classes": ["x", "y", "z"], "num_fc_layers": 1, "num_fc_units": 32, "global_pool": True, "output_stride": 32}}
    outs = {}
    for prec in ("exact", "fp16"):
        mv = Model("swint", bb, hv, "multi_class_topdown").init_xavier_(seed=3, head_scale=1.0)
        mv.to(DEV).set_precision(prec, swint_f16=True)
        outs[prec] = run(mv)
    assert set(outs["exact"]) == {"CenteredInstanceConfmapsHead", "ClassVectorsHead"}
    for k in outs["exact"]:
        assert torch.equal(outs["exact"][k], outs["fp16"][k]), k
    # ConvNeXt in fp16: the eps parameter of layernorm_f16_kernel and the new epilogue forms of gemm_f16_kernel did not move a bit
    cb = {"model_type": None, "arch": {"depths": [1, 2, 1, 1], "channels": [16, 32, 64, 128]}, "in_channels": 1, "kernel_size": 3, "filters_rate": 2, "convs_per_block": 2,
          "up_interpolate": True, "stem_patch_kernel": 4, "stem_patch_stride": 2, "output_stride": 2, "max_stride": 32}
    ch = _heads(5)
    cimg = _u8((2, 1, 64, 96), 11)
    csd = O.init_state_convnext(cb, ch, "single_instance", seed=7, head_scale=1.0, layer_scale=0.5, randomize_affine=True)
    for swin_opt in (0, 1):
        cm = Model("convnext", cb, ch, "single_instance")
        cm.load_state_dict(csd, strict=True)
        cm.to(DEV).set_precision("fp16", convnext_f16=True).set_option("swint_f16", swin_opt)
        got = cm(cimg.to(DEV))["SingleInstanceConfmapsHead"].cpu().contiguous()
        assert L.CNX_KV_F16_GEMM in cm.last_kernels()
        digest = hashlib.sha256(got.numpy().tobytes()).hexdigest()
        print("convnext_f16 sha256", digest)
        assert digest == CONVNEXT_F16_SHA256, swin_opt


def test_hip_backend_use_fp16_eager_and_graph():
    """HipBackend(model, use_fp16=True) on a model whose swint_f16 option is set, eager and as a captured graph: equal bits, within the bar."""
    from sleap_nn_amd.architectures.model import Model
    from sleap_nn_amd.inference.backends import HipBackend

    bb, heads, mt, sd, img, ref, _collect, emu = _case("small")
    outs = {}
    for graph in (False, True):
        m = Model("swint", bb, heads, mt)
        m.load_state_dict(sd, strict=True)
        m.set_option("swint_f16", 1)
        be = HipBackend(m, DEV, use_fp16=True, use_graph=graph)
        first = {k: v.clone() for k, v in be(img).items()}
        outs[graph] = {k: v.clone() for k, v in be(img).items()}  # (graph: a replay)
        torch.cuda.synchronize()
        _assert_f16_route(m)
        for k in first:
            assert torch.equal(first[k], outs[graph][k]), (graph, k)
    for k in ref:
        assert outs[False][k].dtype == torch.float32
        assert torch.equal(outs[False][k], outs[True][k]), k
    _check_heads("small, HipBackend", outs[False], ref, emu)
