"""Swin Transformer backbone, the parts that need no GPU: the plain-torch restatement (tests/swin_ref.py) against an independent
implementation, the wrapper's parameter names and counts, checkpoint loading, output strides and the refusals.

The restatement is compared with HuggingFace transformers' ``SwinLayer`` / ``SwinPatchMerging`` -- an independent implementation of
the same paper, NOT a torchvision pin (torchvision is not installed here; a torchvision-generated golden can be added later).
"""
import math

import pytest
import torch

from tests import swin_ref as R

TINY_ENC = 27_519_354
CLASSIFIER = {"tiny": 769_000, "small": 769_000, "base": 1_025_000}
PUBLISHED = {"tiny": 28_288_354, "small": 49_606_258, "base": 87_768_224}  # torchvision swin_t / swin_s / swin_b


def _bb(**kw):
    bb = {"model_type": None, "arch": {"embed": 32, "depths": [2, 2, 2, 2], "num_heads": [1, 2, 4, 8]}, "in_channels": 1, "patch_size": 4, "window_size": 7,
          "kernel_size": 3, "filters_rate": 2, "convs_per_block": 2, "up_interpolate": True, "stem_patch_stride": 2, "output_stride": 2, "max_stride": 32}
    bb.update(kw)
    return bb


def _heads(n=3, stride=2):
    return {"confmaps": {"part_names": [str(i) for i in range(n)], "sigma": 2.5, "output_stride": stride}}


@pytest.mark.parametrize("H,W,shift", [(10, 13, 0), (10, 13, 3), (14, 21, 3), (8, 8, 3)])
def test_block_restatement_matches_transformers_swin_layer(H, W, shift):
    """Both map sides exceed the window, so both libraries' shift rules agree.  Bar: 1e-5 of the output's scale."""
    from transformers.models.swin.modeling_swin import SwinConfig, SwinLayer

    torch.manual_seed(0)
    C, heads, ws = 64, 2, 7
    cfg = SwinConfig(window_size=ws, layer_norm_eps=1e-5, hidden_act="gelu", mlp_ratio=4.0, qkv_bias=True, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    layer = SwinLayer(cfg, C, (H, W), heads, 0.0, shift).eval()
    for q in layer.parameters():
        torch.nn.init.normal_(q, std=0.3)
    a = layer.attention
    n = "b"
    sd = {
        n + ".norm1.weight": layer.layernorm_before.weight, n + ".norm1.bias": layer.layernorm_before.bias,
        n + ".norm2.weight": layer.layernorm_after.weight, n + ".norm2.bias": layer.layernorm_after.bias,
        n + ".attn.qkv.weight": torch.cat([a.q_proj.weight, a.k_proj.weight, a.v_proj.weight]),
        n + ".attn.qkv.bias": torch.cat([a.q_proj.bias, a.k_proj.bias, a.v_proj.bias]),
        n + ".attn.proj.weight": a.o_proj.weight, n + ".attn.proj.bias": a.o_proj.bias,
        n + ".attn.relative_position_bias_table": a.relative_position_bias.relative_position_bias_table,
        n + ".mlp.0.weight": layer.mlp.fc1.weight, n + ".mlp.0.bias": layer.mlp.fc1.bias,
        n + ".mlp.3.weight": layer.mlp.fc2.weight, n + ".mlp.3.bias": layer.mlp.fc2.bias,
    }
    assert torch.equal(a.relative_position_bias.relative_position_index.flatten(), R.rel_index(ws))
    x = torch.randn(2, H, W, C)
    with torch.no_grad():
        want = layer(x.view(2, H * W, C), (H, W))
        want = want[0] if isinstance(want, tuple) else want
        got = R.swin_block(sd, n, x, ws, heads, shift).view(2, H * W, C)
    scale = want.abs().max().item()
    err = (got - want).abs().max().item()
    print(f"{H}x{W} shift {shift}: max diff {err:.3g} at scale {scale:.3g}")
    assert err <= 1e-5 * scale, (err, scale)


def test_patch_merging_restatement_matches_transformers():
    from transformers.models.swin.modeling_swin import SwinPatchMerging

    torch.manual_seed(1)
    for H, W in ((6, 10), (7, 9)):  # even, and odd in both axes (both pad right / bottom with zeros)
        C = 32
        pm = SwinPatchMerging(C).eval()  # (transformers 5: the constructor takes the channel count only)
        assert pm.norm.eps == 1e-5
        for q in pm.parameters():
            torch.nn.init.normal_(q, std=0.3)
        x = torch.randn(2, H, W, C)
        with torch.no_grad():
            want = pm(x.view(2, H * W, C), (H, W))
            got = R.patch_merging(x, pm.norm.weight, pm.norm.bias, pm.reduction.weight).reshape(2, -1, 2 * C)
        scale = want.abs().max().item()
        err = (got - want).abs().max().item()
        print(f"merge {H}x{W}: max diff {err:.3g} at scale {scale:.3g}")
        assert err <= 1e-5 * scale, (err, scale)


def test_relative_position_index_is_the_canonical_one():
    from sleap_nn_amd.architectures.swint import relative_position_index

    for ws in range(2, 9):
        idx = relative_position_index(ws)
        assert idx.dtype == torch.int64 and idx.shape == (ws**4,)
        assert torch.equal(idx, R.rel_index(ws))
        # what the kernel computes from coordinates
        t = torch.arange(ws * ws)
        ty, tx = t // ws, t % ws
        want = (ty[:, None] - ty[None, :] + ws - 1) * (2 * ws - 1) + (tx[:, None] - tx[None, :] + ws - 1)
        assert torch.equal(idx.view(ws * ws, ws * ws), want)


@pytest.mark.parametrize("variant", ["tiny", "small", "base"])
def test_param_shapes_reproduce_the_published_totals(variant):
    from sleap_nn_amd.architectures.swint import SwinTWrapper

    net = SwinTWrapper.from_config(_bb(model_type=variant, arch=None, in_channels=3))
    enc = sum(math.prod(s) for k, s in net.param_shapes.items() if k.startswith("backbone.enc."))
    assert enc + CLASSIFIER[variant] == PUBLISHED[variant], enc
    if variant == "tiny":
        assert enc == TINY_ENC
        gray = SwinTWrapper.from_config(_bb(model_type="tiny", arch=None, in_channels=1))
        assert sum(math.prod(s) for k, s in gray.param_shapes.items() if k.startswith("backbone.enc.")) == 27_516_282


def test_tiny_key_set_follows_torchvision_names():
    from sleap_nn_amd.architectures.swint import SwinTWrapper

    net = SwinTWrapper.from_config(_bb(model_type="tiny", arch=None, in_channels=3))
    want = {"features.0.0.weight", "features.0.0.bias", "features.0.2.weight", "features.0.2.bias", "norm.weight", "norm.bias"}
    for fi, (depth, _) in zip((1, 3, 5, 7), zip([2, 2, 6, 2], [3, 6, 12, 24])):
        for j in range(depth):
            for leaf in ("norm1.weight", "norm1.bias", "attn.qkv.weight", "attn.qkv.bias", "attn.proj.weight", "attn.proj.bias", "attn.relative_position_bias_table",
                         "norm2.weight", "norm2.bias", "mlp.0.weight", "mlp.0.bias", "mlp.3.weight", "mlp.3.bias"):
                want.add(f"features.{fi}.{j}.{leaf}")
    for fi in (2, 4, 6):
        want |= {f"features.{fi}.norm.weight", f"features.{fi}.norm.bias", f"features.{fi}.reduction.weight"}
    got = {k[len("backbone.enc."):] for k in net.param_shapes if k.startswith("backbone.enc.")}
    assert got == want
    assert not any("relative_position_index" in k for k in net.param_shapes)
    assert {k[len("backbone.enc."):] for k in net.buffers} == {f"features.{fi}.{j}.attn.relative_position_index" for fi, d in zip((1, 3, 5, 7), [2, 2, 6, 2]) for j in range(d)}
    assert net.param_shapes["backbone.enc.features.1.0.attn.relative_position_bias_table"] == (169, 3)
    assert net.param_shapes["backbone.enc.features.6.norm.weight"] == (1536,)


def test_load_state_dict_strict_checks_the_index_buffer():
    from sleap_nn_amd.architectures.model import Model

    bb, heads = _bb(), _heads()
    sd = R.init_state_swint(bb, heads, "single_instance", seed=3)
    m = Model("swint", bb, heads, "single_instance")
    n_params = m.num_parameters()
    m.load_state_dict({"model." + k: v for k, v in sd.items()}, strict=True)  # index buffers included, LightningModule prefix
    assert set(m.state_dict()) == set(sd)
    assert m.flat_params().numel() == n_params == sum(v.numel() for k, v in sd.items() if not k.endswith("relative_position_index"))
    key = "backbone.enc.features.3.1.attn.relative_position_index"
    bad = dict(sd)
    bad[key] = sd[key].clone()
    bad[key][5] += 1
    with pytest.raises(RuntimeError, match="relative_position_index"):
        m.load_state_dict(bad, strict=True)
    missing = {k: v for k, v in sd.items() if k != "backbone.enc.norm.weight"}
    with pytest.raises(RuntimeError, match="backbone.enc.norm.weight"):
        m.load_state_dict(missing, strict=True)
    extra = dict(sd)
    extra["backbone.enc.features.1.0.layer_scale"] = torch.ones(32)
    with pytest.raises(RuntimeError, match="layer_scale"):
        m.load_state_dict(extra, strict=True)


def test_output_strides_and_shapes_of_the_wrapper():
    """What the reference's tests/architectures/test_swint.py asserts, as expected values: tiny at 384 x 384, output_stride 2, gives five decoder outputs whose
    last is (1, 96, 192, 192); max_stride = stem_patch_stride * 16."""
    from sleap_nn_amd.architectures.swint import SwinTWrapper

    net = SwinTWrapper.from_config(_bb(model_type="tiny", arch=None, in_channels=1, output_stride=2))
    assert net.max_stride == 32 and net.max_channels == 1536
    assert net.decoder_stride_to_filters == {32: 1536, 16: 768, 8: 384, 4: 192, 2: 96}
    assert sorted(net.decoder_slot_of_stride) == [2, 4, 8, 16]
    # the plain-torch restatement at a small width produces the same stride ladder with real tensors
    bb, heads = _bb(output_stride=2), _heads()
    sd = R.init_state_swint(bb, heads, "single_instance", seed=2)
    out = R.swint_forward(sd, bb, torch.rand(1, 1, 64, 96))
    assert out["strides"] == [16, 8, 4, 2]
    assert [tuple(o.shape) for o in out["outputs"]] == [(1, 256, 4, 6), (1, 128, 8, 12), (1, 64, 16, 24), (1, 32, 32, 48)]
    assert tuple(out["middle_output"].shape) == (1, 512, 2, 3)
    s4 = SwinTWrapper.from_config(_bb(model_type="tiny", arch=None, stem_patch_stride=4, output_stride=4))
    assert s4.max_stride == 64 and sorted(s4.decoder_slot_of_stride) == [4, 8, 16, 32]


def test_op_table_counts_the_attention_flops():
    from sleap_nn_amd import _lib as L
    from sleap_nn_amd.architectures.model import Model

    m = Model("swint", _bb(), _heads(), "single_instance")
    rows = [r for r in m.op_table(2, 64, 96) if r["kind"] == L.OP_WINDOW_ATTN]
    assert len(rows) == 8
    assert rows[0]["flops"] == 4.0 * 49 * 32 * (32 * 48 * 2)  # 4 N d per token and head, one head of 32 channels
    assert rows[-1]["flops"] == 4.0 * 49 * 32 * 8 * (4 * 6 * 2)
    merges = [r for r in m.op_table(2, 64, 96) if r["kind"] == L.OP_PATCH_MERGE]
    assert [r["out_hw"] for r in merges] == [(16, 24), (8, 12), (4, 6)]


def test_refusals():
    from sleap_nn_amd.architectures.model import Model, get_backbone

    with pytest.raises(ValueError, match="num_heads"):
        get_backbone("swint", _bb(arch={"embed": 48, "depths": [2, 2, 2, 2], "num_heads": [1, 2, 4, 8]}))  # head dimension 48
    with pytest.raises(ValueError, match="window_size"):
        get_backbone("swint", _bb(window_size=9))
    with pytest.raises(ValueError, match="block_contraction"):
        get_backbone("swint", _bb(block_contraction=True))
    with pytest.raises(ValueError, match="kernel_size"):
        get_backbone("swint", _bb(kernel_size=5))
    with pytest.raises(NotImplementedError, match="pretrained"):
        get_backbone("pretrained", _bb())
    m = Model("swint", _bb(), _heads(), "single_instance")
    with pytest.raises(NotImplementedError, match="swint"):
        m.train()
    assert m.eval() is m and m.set_precision("fp16").precision == "fp16"  # accepted; the encoder stays exact (tests/test_gpu_swint.py)


def test_init_xavier_covers_the_swin_parameters():
    from sleap_nn_amd.architectures.model import Model

    m = Model("swint", _bb(), _heads(), "single_instance").init_xavier_(seed=3)
    sd = m.state_dict()
    assert torch.equal(sd["backbone.enc.features.2.norm.weight"], torch.ones(128)) and torch.equal(sd["backbone.enc.norm.weight"], torch.ones(256))
    assert float(sd["backbone.enc.features.1.0.attn.relative_position_bias_table"].abs().max()) > 0 and float(sd["backbone.enc.features.2.reduction.weight"].abs().max()) > 0
    assert torch.equal(sd["backbone.enc.features.1.1.attn.relative_position_index"], R.rel_index(7))
