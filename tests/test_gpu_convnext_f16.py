"""ConvNeXt inference on the fp16 matrix pipe (``set_precision("fp16", convnext_f16=True)``; convnext_f16_kernels.hip) against the fp32 oracle.

Bar: ``FP16_ATOL`` = 5e-3, the reference's own fp16 bar (tests/inference/test_cuda.py:54-55) and the one tests/test_gpu_f16_pipe.py uses, applied as
tests/test_gpu_convnext.py::_run applies its tolerance: max |got - ref| / max(1, max |ref|).  tools/convnext_f16_emulation.py predicts ~1e-3 for the
storage the device uses (everything in fp16, the residual stream included).
"""
import functools

import pytest
import torch

from oracle import cpu_ref as O

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FP16_ATOL = 5e-3
PLAN_ATOL = 2e-3  # inference plan vs keep-everything plan: a few fp16 ulps at the heads (the figure tests/test_gpu_f16_pipe.py uses for the same comparison)

CONFIGS = [
    ([16, 32, 64, 128], [1, 2, 1, 1], 2, 2, (64, 96), 2),      # multiples of 16: every width but 64 / 128 is padded to 32
    ([24, 40, 72, 136], [2, 1, 1, 1], 2, 4, (64, 64), 3),      # padded channels everywhere: LayerNorm must ignore the pad lanes, odd N blocks
    ([32, 64, 128, 256], [1, 1, 2, 1], 4, 1, (128, 64), 1),    # stem stride 4: two decoder blocks without a skip
    ([96, 192, 384, 768], [1, 1, 1, 1], 2, 2, (96, 160), 2),   # the tiny variant's widths (3 / 6 / 12 / 24 N blocks, K up to 3072)
]


def _bb(**kw):
    bb = {"model_type": None, "arch": None, "in_channels": 1, "kernel_size": 3, "filters_rate": 2, "convs_per_block": 2, "up_interpolate": True,
          "stem_patch_kernel": 4, "stem_patch_stride": 2, "output_stride": 2, "max_stride": 32}
    bb.update(kw)
    return bb


def _heads(n, stride):
    return {"confmaps": {"part_names": [str(i) for i in range(n)], "sigma": 2.5, "output_stride": stride}}


@functools.lru_cache(maxsize=None)
def _case(i, seed=7):
    """Configuration i of CONFIGS: (bb, heads, model type, state dict, image, oracle heads, oracle activations) -- computed once, shared, never modified."""
    channels, depths, ss, os_, hw, batch = CONFIGS[i]
    bb = _bb(arch={"depths": depths, "channels": channels}, stem_patch_stride=ss, output_stride=os_)
    heads = _heads(5, os_)
    img = torch.randint(0, 256, (batch, 1, hw[0], hw[1]), dtype=torch.uint8, generator=torch.Generator().manual_seed(11))
    sd = O.init_state_convnext(bb, heads, "single_instance", seed=seed, head_scale=1.0, layer_scale=0.5, randomize_affine=True)
    collect = {}
    ref = O.model_forward(sd, bb, heads, "single_instance", img, collect=collect, backbone="convnext")
    return bb, heads, "single_instance", sd, img, ref, collect


def _model(bb, heads, mt, sd, precision="fp16", keep=False):
    from sleap_nn_amd.architectures.model import Model

    m = Model("convnext", bb, heads, mt)
    m.load_state_dict(sd, strict=True)
    m.to(DEV).set_keep_activations(keep)
    return m.set_precision(precision, convnext_f16=True)


def _err(got, ref):
    return (got.cpu() - ref).abs().max().item() / max(1.0, ref.abs().max().item())


def _assert_f16_route(m):
    """Every ConvNeXt op of the last forward ran a kernel of convnext_f16_kernels.hip, every 3x3 conv an fp16 conv kernel: no fp32 row GEMM, no fp32 MLP kernel."""
    from sleap_nn_amd import _lib as L

    want = {L.OP_PATCH_STEM: {L.CNX_KV_F16_STEM}, L.OP_DWCONV: {L.CNX_KV_F16_DW}, L.OP_LAYERNORM: {L.CNX_KV_F16_LN, L.KV_FUSED}, L.OP_LINEAR: {L.CNX_KV_F16_GEMM},
            L.OP_PATCH_CONV: {L.CNX_KV_F16_GEMM}, L.OP_GELU: {L.CNX_KV_F16_ELTWISE}, L.OP_SCALE_ADD: {L.CNX_KV_F16_ELTWISE}, L.OP_CONV: {L.KV_F16, L.KV_F16_ROWS, L.KV_F16_BLOCK, L.KV_FUSED}}
    kv = list(m.last_kernels())
    assert m.get_option("conv_precision") == 2.0
    for op, code in zip(m.ops, kv):
        if op.kind in want:
            assert code in want[op.kind], (op.label, op.kind, code)
    assert L.KV_ROWGEMM not in kv and L.KV_MLP not in kv, kv
    return kv


def _pad_channels_are_zero(m, batch):
    """Every activation slot of the last (keep-everything) forward, read straight from the workspace as (pixels, Cp) halves: the channels past the true count are exact zeros."""
    from sleap_nn_amd import _lib as L

    ws = m._workspace
    seen = 0
    for op_i, _launch, is_dst, slot, off, nbytes in m.last_ranges():
        if not is_dst or slot < 0:
            continue
        op = m.ops[op_i]
        c = op.cin0 if op.kind in (L.OP_POOL, L.OP_UPSAMPLE) else op.cout
        if slot != op.dst:
            continue
        cp = (c + 31) // 32 * 32
        assert nbytes % (2 * cp) == 0, (op.label, nbytes, cp)
        t = ws[off:off + nbytes].view(torch.float16).view(-1, cp)
        assert t.shape[0] % batch == 0
        if cp > c:
            assert bool((t[:, c:] == 0).all()), (op.label, "pad channels", float(t[:, c:].abs().max()))
            seen += 1
        assert bool(torch.isfinite(t.float()).all()), op.label
    return seen


@pytest.mark.parametrize("i", range(len(CONFIGS)))
def test_convnext_f16_forward_matches_oracle_on_the_fp16_route(i):
    """Keep-everything plan: every labelled block activation and every head within the bar, the new kernel codes on every ConvNeXt op, a second forward gives the same bits."""
    bb, heads, mt, sd, img, ref, collect = _case(i)
    m = _model(bb, heads, mt, sd, keep=True)
    out = {k: v.clone() for k, v in m(img.to(DEV)).items()}
    torch.cuda.synchronize()
    kv = _assert_f16_route(m)
    from sleap_nn_amd import _lib as L

    assert L.KV_FUSED not in [c for op, c in zip(m.ops, kv) if op.kind == L.OP_LAYERNORM]  # (nothing is fused away in the plan that keeps every activation)
    worst = {}
    for name, t in collect.items():
        if name not in m.backbone.labels:
            continue
        worst[name] = _err(m.read_activation(name, t.shape[0], t.shape[-2:]), t)
    for k, t in ref.items():
        assert out[k].shape == t.shape
        worst[k] = _err(out[k], t)
    print({k: f"{v:.2e}" for k, v in worst.items()})
    bad = {k: v for k, v in worst.items() if not v <= FP16_ATOL}
    assert not bad, bad
    again = m(img.to(DEV))
    for k in out:
        assert torch.equal(out[k], again[k]), (k, "not repeatable")


def test_convnext_f16_rows_and_channels_off_the_tile_and_zero_pad_channels():
    """M no multiple of any row tile at every stage (gray (1, 1, 32, 96) into an RGB model, depths 1/1/1/1), and the padded-width configuration: within the bar, and
    the pad channels of every kept activation read back as exact zeros."""
    bb = _bb(arch={"depths": [1, 1, 1, 1], "channels": [16, 32, 64, 128]}, in_channels=3)
    heads = _heads(3, 2)
    img = torch.randint(0, 256, (1, 1, 32, 96), dtype=torch.uint8, generator=torch.Generator().manual_seed(5))
    sd = O.init_state_convnext(bb, heads, "single_instance", seed=7, head_scale=1.0, layer_scale=0.5, randomize_affine=True)
    ref = O.model_forward(sd, bb, heads, "single_instance", img, backbone="convnext")
    m = _model(bb, heads, "single_instance", sd, keep=True)
    out = m(img.to(DEV))
    torch.cuda.synchronize()
    _assert_f16_route(m)
    for k, t in ref.items():
        e = _err(out[k], t)
        print(k, f"{e:.2e}")
        assert e <= FP16_ATOL, (k, e)
    assert _pad_channels_are_zero(m, 1) >= 4  # 16-channel stage: stem, LayerNorm, depthwise, LayerNorm, block output ... all padded to 32
    bb2, heads2, mt2, sd2, img2, ref2, _ = _case(1)
    m2 = _model(bb2, heads2, mt2, sd2, keep=True)
    out2 = m2(img2.to(DEV))
    torch.cuda.synchronize()
    for k, t in ref2.items():
        assert _err(out2[k], t) <= FP16_ATOL, k
    assert _pad_channels_are_zero(m2, img2.shape[0]) >= 10  # 24 / 40 / 72 / 136 and their 4x hidden widths: every encoder slot is padded


@pytest.mark.parametrize("i", [0, 1, 3])
def test_convnext_f16_inference_plan_agrees_with_the_keep_everything_plan(i):
    """workspace_reuse 1 (depthwise + LayerNorm in one launch, shared slots, folded bilinears, heads in conv epilogues) vs the plan that keeps every tensor: a few fp16 ulps."""
    from sleap_nn_amd import _lib as L

    bb, heads, mt, sd, img, ref, _ = _case(i)
    keep = _model(bb, heads, mt, sd, keep=True)
    a = {k: v.clone() for k, v in keep(img.to(DEV)).items()}
    inf = _model(bb, heads, mt, sd, keep=False)
    b = inf(img.to(DEV))
    torch.cuda.synchronize()
    assert inf.get_option("workspace_reuse") == 1.0
    kv = _assert_f16_route(inf)
    ln = [c for op, c in zip(inf.ops, kv) if op.kind == L.OP_LAYERNORM]
    assert L.KV_FUSED in ln and L.CNX_KV_F16_LN in ln, ln  # CNBlock LayerNorms ride in the depthwise kernel; the stem's and the downsampling ones stand alone
    for k, t in ref.items():
        scale = max(1.0, t.abs().max().item())
        d = (a[k] - b[k]).abs().max().item() / scale
        print(k, f"plans differ by {d:.2e}; inference plan vs oracle {_err(b[k], t):.2e}")
        assert d <= PLAN_ATOL, (k, d)
        assert _err(b[k], t) <= FP16_ATOL, k


def test_convnext_f16_weight_images_follow_live_parameters():
    """A handle created from state A and re-bound to state B's device arena gives, in fp16, the bits of a fresh handle created from B: the fp16 weight images are rebuilt."""
    from sleap_nn_amd.architectures.model import Model

    bb, heads, mt, sd_a, img, _ref, _ = _case(0)
    sd_b = O.init_state_convnext(bb, heads, mt, seed=8, head_scale=1.0, layer_scale=0.4, randomize_affine=True)
    fresh = _model(bb, heads, mt, sd_b)
    want = {k: v.clone() for k, v in fresh(img.to(DEV)).items()}
    donor = Model("convnext", bb, heads, mt)
    donor.load_state_dict(sd_b, strict=True)
    live = _model(bb, heads, mt, sd_a)  # (the handle is created from A's host copy -- fp16 images included --, then re-packed from the arena: ph_model_set_params)
    live.bind_live_params(donor.flat_params().to(DEV))
    got = live(img.to(DEV))
    torch.cuda.synchronize()
    _assert_f16_route(live)
    from_a = _model(bb, heads, mt, sd_a)(img.to(DEV))
    for k in want:
        assert torch.equal(got[k], want[k]), (k, (got[k] - want[k]).abs().max().item())
        assert not torch.equal(from_a[k], want[k]), k  # (A and B do differ)


def test_convnext_f16_switching_precisions_on_one_handle():
    """fp16 -> exact -> fp16 on one handle: the exact forward equals a fresh exact handle bit for bit, the two fp16 forwards are equal."""
    bb, heads, mt, sd, img, _ref, _ = _case(0)
    m = _model(bb, heads, mt, sd)
    f1 = {k: v.clone() for k, v in m(img.to(DEV)).items()}
    _assert_f16_route(m)
    m.set_precision("exact")
    ex = {k: v.clone() for k, v in m(img.to(DEV)).items()}
    assert m.get_option("conv_precision") == 0.0
    m.set_precision("fp16")
    f2 = m(img.to(DEV))
    _assert_f16_route(m)
    fresh = _model(bb, heads, mt, sd, precision="exact")
    want = fresh(img.to(DEV))
    torch.cuda.synchronize()
    for k in want:
        assert torch.equal(ex[k], want[k]), k
        assert torch.equal(f1[k], f2[k]), k
        assert not torch.equal(f1[k], ex[k]), k


def test_programs_that_must_stay_exact():
    """A class-vector head (global max pool, softmax), the split precision and a training program keep a ConvNeXt model on the exact path, bit for bit --
    and so does "fp16" while the handle option convnext_f16 is at its default."""
    from sleap_nn_amd import _lib as L
    from sleap_nn_amd.architectures.model import Model

    bb, heads, mt, sd, img, _ref, _ = _case(0)
    x = img.to(DEV)

    def run(model, **kw):
        out = {k: v.clone() for k, v in model(x).items()}
        kv = list(model.last_kernels())
        assert not ({L.CNX_KV_F16_STEM, L.CNX_KV_F16_DW, L.CNX_KV_F16_LN, L.CNX_KV_F16_GEMM, L.CNX_KV_F16_ELTWISE, L.KV_F16, L.KV_F16_ROWS} & set(kv)), kv
        return out

    exact = run(_model(bb, heads, mt, sd, precision="exact"))
    split = run(_model(bb, heads, mt, sd, precision="split"))
    default = Model("convnext", bb, heads, mt)
    default.load_state_dict(sd, strict=True)
    dflt = run(default.to(DEV).set_precision("fp16"))  # (convnext_f16 untouched: 0)
    for k in exact:
        assert torch.equal(split[k], exact[k]) and torch.equal(dflt[k], exact[k]), k
    tr_e = _model(bb, heads, mt, sd, precision="exact").train()
    tr_f = _model(bb, heads, mt, sd, precision="fp16").train()
    a, b = run(tr_e), run(tr_f)
    assert tr_f.get_option("conv_precision") == 0.0
    for k in a:
        assert torch.equal(a[k], b[k]), k
    # multi_class_topdown: confidence maps + a class-vector head on the middle feature
    hv = {"confmaps": {"part_names": ["a", "b", "c"], "anchor_part": None, "sigma": 2.5, "output_stride": 2},
          "class_vectors": {"classes": ["x", "y", "z"], "num_fc_layers": 1, "num_fc_units": 32, "global_pool": True, "output_stride": 32}}
    outs = {}
    for prec in ("exact", "fp16"):
        mv = Model("convnext", bb, hv, "multi_class_topdown").init_xavier_(seed=3, head_scale=1.0)
        mv.to(DEV).set_precision(prec, convnext_f16=True)
        outs[prec] = run(mv)
    assert set(outs["exact"]) == {"CenteredInstanceConfmapsHead", "ClassVectorsHead"}
    for k in outs["exact"]:
        assert torch.equal(outs["exact"][k], outs["fp16"][k]), k


def test_hip_backend_use_fp16_eager_and_graph():
    """HipBackend(model, use_fp16=True) on a model whose convnext_f16 option is set, eager and as a captured graph: equal bits, within the bar of the oracle."""
    from sleap_nn_amd.architectures.model import Model
    from sleap_nn_amd.inference.backends import HipBackend

    bb, heads, mt, sd, img, ref, _ = _case(0)
    outs = {}
    for graph in (False, True):
        m = Model("convnext", bb, heads, mt)
        m.load_state_dict(sd, strict=True)
        m.set_option("convnext_f16", 1)
        be = HipBackend(m, DEV, use_fp16=True, use_graph=graph)
        first = {k: v.clone() for k, v in be(img).items()}
        outs[graph] = {k: v.clone() for k, v in be(img).items()}  # (graph: a replay)
        torch.cuda.synchronize()
        _assert_f16_route(m)
        for k in first:
            assert torch.equal(first[k], outs[graph][k]), (graph, k)
    for k, t in ref.items():
        assert outs[False][k].dtype == torch.float32
        assert torch.equal(outs[False][k], outs[True][k]), k
        assert _err(outs[False][k], t) <= FP16_ATOL, k


def test_convnext_tiny_rgb_float_crop_in_fp16():
    """The whole ConvNeXt-tiny (depths 3/3/9/3: 18 blocks of fp16-stored residual) on one float RGB 96 x 96 crop, 13 nodes: heads within the bar."""
    bb = _bb(model_type="tiny", in_channels=3, output_stride=2)
    heads = _heads(13, 2)
    img = torch.rand((1, 3, 96, 96), generator=torch.Generator().manual_seed(3))
    sd = O.init_state_convnext(bb, heads, "centered_instance", seed=7, head_scale=1.0, layer_scale=0.3, randomize_affine=True)
    ref = O.model_forward(sd, bb, heads, "centered_instance", img, backbone="convnext")
    m = _model(bb, heads, "centered_instance", sd)
    out = m(img.to(DEV))
    torch.cuda.synchronize()
    _assert_f16_route(m)
    for k, t in ref.items():
        e = _err(out[k], t)
        print(k, f"{e:.2e}")
        assert e <= FP16_ATOL, (k, e)
