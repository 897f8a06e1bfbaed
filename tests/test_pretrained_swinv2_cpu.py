"""The Swinv2 family of the ``pretrained`` backbone without a GPU: architecture resolution and its refusals, the per-stage window / shift derivation, the coordinate
table and the ``16 sigmoid`` bias form, the program's parameter names and order against ``Swinv2Backbone.state_dict()``, the derived tensors the library is handed, and
tests/swinv2_ref.py against the reference's own outputs (tests/golden/pretrained_swinv2_*.npz, written by tools/gen_pretrained_swinv2_golden.py) and against
``transformers`` where it is installed.

The weights are drawn, not stored (tests/_swinv2_cases.draw_state, from the seed in the golden).  The bar for the restatement is that of tests/test_pretrained_cpu.py:
1e-5 of each map's scale."""
import glob
import json
import math
import os
import re

import numpy as np
import pytest
import torch

from tests import _swinv2_cases as SC
from tests import swinv2_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
ENC = "backbone.enc"
HEAD = "SingleInstanceConfmapsHead"
W8_256 = "microsoft/swinv2-tiny-patch4-window8-256"


def bb_of(name, model_name, allow=True):
    return SC.backbone_config(name, model_name, allow)


def heads_of(name):
    return SC.head_config(name)


def arch_of(name, **over):
    return SC.hf_json(SC.FIXTURES[name], **over)


def hf_dir(name, tmp_path, **over):
    """A directory with the fixture's ``config.json``, written here (settings only)."""
    d = tmp_path / ("hf_" + name + "_".join(sorted(over)))
    d.mkdir(exist_ok=True)
    with open(d / "config.json", "w") as f:
        json.dump(arch_of(name, **over), f)
    return str(d)


def new_model(name, tmp_path, **bb_over):
    from sleap_nn_amd.architectures.model import Model

    return Model("pretrained", dict(bb_of(name, hf_dir(name, tmp_path)), **bb_over), heads_of(name), "single_instance")


def state_of(model, seed):
    """The seeded state dict over the model's parameter shapes + its image statistics as they stand."""
    sd = {k: torch.from_numpy(v) for k, v in SC.draw_state(model.param_shapes, seed).items()}
    sd.update({k: v.clone() for k, v in model.buffers.items()})
    return sd


_CACHE = {}


def golden(name):
    """The reference's outputs of a fixture (main file + the layer files as one dict), loaded once."""
    if name not in _CACHE:
        g = {}
        stem = os.path.join(GOLD, f"pretrained_swinv2_{name.lower()}")
        for f in [stem + ".npz"] + sorted(glob.glob(stem + "_layers*.npz")):
            z = np.load(f)
            g.update({k: z[k] for k in z.files})
        g["frames"] = SC.frames(name)
        _CACHE[name] = g
    return _CACHE[name]


_STATES = {}


def golden_state(name, tmp_path):
    """The state dict the golden was computed with (drawn once per fixture)."""
    if name not in _STATES:
        _STATES[name] = state_of(new_model(name, tmp_path), int(golden(name)["seed"]))
    return _STATES[name]


def write_run_dir(path, name, sd):
    """A run directory of fixture ``name``: best.ckpt (Lightning keys), training_config.yaml, hf_config/config.json."""
    import yaml

    os.makedirs(os.path.join(path, "hf_config"), exist_ok=True)
    with open(os.path.join(path, "hf_config", "config.json"), "w") as f:
        json.dump(arch_of(name), f)
    torch.save({"state_dict": {"model." + k: v.clone() for k, v in sd.items()}}, os.path.join(path, "best.ckpt"))
    heads = {k: None for k in ("single_instance", "centroid", "centered_instance", "bottomup", "multi_class_bottomup", "multi_class_topdown",
                               "bottomup_segmentation", "semantic_segmentation", "centered_instance_segmentation")}
    heads["single_instance"] = heads_of(name)
    pre = {"ensure_rgb": True, "ensure_grayscale": False, "max_height": None, "max_width": None, "scale": 1.0, "crop_size": None}
    cfg = {"data_config": {"preprocessing": pre, "skeletons": [{"name": "s", "nodes": [{"name": n} for n in SC.PARTS], "edges": []}]},
           "model_config": {"backbone_config": {"unet": None, "convnext": None, "swint": None, "pretrained": bb_of(name, "hf_config", allow=False)}, "head_configs": heads},
           "trainer_config": {"run_name": os.path.basename(str(path))}, "name": "", "description": "", "sleap_nn_version": "0.0.1"}
    with open(os.path.join(path, "training_config.yaml"), "w") as f:
        yaml.safe_dump(cfg, f, sort_keys=False)
    return str(path)


def rel(got, want):
    want = torch.as_tensor(want)
    return (torch.as_tensor(got) - want).abs().max().item() / max(1e-30, want.abs().max().item())


# ---- resolution, windows and shifts

def test_resolution_from_config_json_and_table(tmp_path):
    from sleap_nn_amd.architectures import pretrained as P

    for name, c in SC.FIXTURES.items():
        a = P.resolve_architecture(hf_dir(name, tmp_path), allow_swinv2=True)
        assert a["family"] == "swinv2" and a["patch_size"] == 4 and a["hidden_sizes"] == [32, 64, 128, 256]
        assert (a["embed_dim"], a["depths"], a["num_heads"], a["window_size"], a["image_size"], a["pretrained_window_sizes"], a["mlp_ratio"], a["layer_norm_eps"]) == \
            (32, c["depths"], c["num_heads"], c["window_size"], [c["image_size"]] * 2, c["pretrained_window_sizes"], c["mlp_ratio"], 1e-5)
        assert a["drop_path_rate"] == 0.1 and a["qkv_bias"] is True
    want = {"tiny": (96, [2, 2, 6, 2], [3, 6, 12, 24]), "small": (96, [2, 2, 18, 2], [3, 6, 12, 24]), "base": (128, [2, 2, 18, 2], [4, 8, 16, 32])}
    for size, (e, d, h) in want.items():
        a = P.resolve_architecture(f"microsoft/swinv2-{size}-patch4-window8-256", allow_swinv2=True)
        assert (a["family"], a["embed_dim"], a["depths"], a["num_heads"], a["window_size"], a["image_size"], a["pretrained_window_sizes"]) == ("swinv2", e, d, h, 8, [256, 256], [0, 0, 0, 0])
    pair = P.resolve_architecture(hf_dir("A", tmp_path, image_size=[64, 96]), allow_swinv2=True)
    assert pair["image_size"] == [64, 96]
    bbn = P.PretrainedBackbone.from_config({"model_name": W8_256, "output_stride": 4, "allow_swinv2": True})
    assert bbn.family == "swinv2" and bbn.channels == [96, 192, 384, 768] and bbn.max_stride == 32 and bbn.max_channels == 768
    assert P.resolve_architecture("facebook/convnextv2-atto-1k-224", allow_swinv2=True)["family"] == "convnextv2"  # the opt-in changes nothing else


def test_tiny_row_is_the_installed_default():
    tr = pytest.importorskip("transformers")
    from sleap_nn_amd.architectures import pretrained as P

    c = tr.Swinv2Config()
    a = P.resolve_architecture("microsoft/swinv2-tiny-patch4-window7-224", allow_swinv2=True)
    assert (a["embed_dim"], a["depths"], a["num_heads"], a["window_size"], a["image_size"][0], a["patch_size"]) == (c.embed_dim, list(c.depths), list(c.num_heads), c.window_size, c.image_size, c.patch_size)
    assert (a["mlp_ratio"], a["layer_norm_eps"], a["pretrained_window_sizes"]) == (c.mlp_ratio, c.layer_norm_eps, list(c.pretrained_window_sizes))
    assert c.hidden_act == "gelu" and c.qkv_bias and not c.use_absolute_embeddings


def test_window_and_shift_follow_the_config_image_size():
    from sleap_nn_amd.architectures import pretrained as P

    assert P.swinv2_windows(64, 4, 4) == [(4, 2), (4, 2), (4, 0), (2, 0)]      # fixture A: stage 3 unshifted at window 4, stage 4 shrinks to window 2
    assert P.swinv2_windows(224, 4, 7) == [(7, 3), (7, 3), (7, 3), (7, 0)]    # fixture B
    assert P.swinv2_windows(256, 4, 8) == [(8, 4), (8, 4), (8, 4), (8, 0)]    # the published window8-256 models run stage 4 unshifted
    assert P.swinv2_windows([256, 512], 4, 8) == P.swinv2_windows(256, 4, 8)  # (HuggingFace keeps the height axis' values)
    assert R.windows_of(SC.hf_json(SC.FIXTURES["A"])) == P.swinv2_windows(64, 4, 4)
    bbn = P.PretrainedBackbone.from_config({"model_name": W8_256, "output_stride": 4, "allow_swinv2": True})
    att = [o for o in bbn.ops if o.kind == P.L.OP_WINDOW_ATTN_V2]
    assert [(o.ksize, o.cmid) for o in att] == [(8, 0), (8, 4)] * 5 + [(8, 0), (8, 0)] and [o.cin1 for o in att] == [3] * 2 + [6] * 2 + [12] * 6 + [24] * 2


@pytest.mark.parametrize("name", ["A", "B", "W8"])
def test_window_and_shift_equal_the_installed_layers(name):
    tr = pytest.importorskip("transformers")
    from sleap_nn_amd.architectures import pretrained as P

    arch = arch_of(name)
    enc = tr.Swinv2Backbone(tr.Swinv2Config(**{k: v for k, v in arch.items() if k != "model_type"}))
    mine = P.swinv2_windows(arch["image_size"], 4, arch["window_size"])
    for si, stage in enumerate(enc.encoder.layers):
        for j, blk in enumerate(stage.blocks):
            assert (blk.window_size, blk.shift_size) == (mine[si][0], mine[si][1] if j % 2 else 0), (si, j)


# ---- coordinate table, bias form, logit scale

@pytest.mark.parametrize("window,pretrained", [(2, 0), (4, 0), (7, 6), (8, 0), (7, 0), (4, 12)])
def test_coords_table_and_bias_form_equal_the_installed_attention(window, pretrained):
    tr = pytest.importorskip("transformers")
    from transformers.models.swinv2.modeling_swinv2 import Swinv2SelfAttention

    from sleap_nn_amd.architectures import pretrained as P

    heads = 3
    att = Swinv2SelfAttention(tr.Swinv2Config(), dim=96, num_heads=heads, window_size=window, pretrained_window_size=[pretrained, pretrained])
    mine = P.swinv2_coords_table(window, pretrained)
    assert mine.dtype == torch.float32 and torch.equal(mine, att.relative_coords_table.view(-1, 2))  # the same float32 operations: the same bits
    assert torch.equal(mine, R.coords_table(window, pretrained).view(-1, 2))
    mlp = "attention.continuous_position_bias_mlp"
    w = {k: torch.from_numpy(SC.draw_tensor(f"x.blocks.1.{mlp}.{k}", s, 9)) for k, s in (("0.weight", (512, 2)), ("0.bias", (512,)), ("2.weight", (heads, 512)))}
    att.continuous_position_bias_mlp.load_state_dict(w)
    att = att.double()
    N = window * window
    with torch.no_grad():
        t = att.continuous_position_bias_mlp(att.relative_coords_table).view(-1, heads)
        want = 16 * torch.sigmoid(t[att.relative_position_index.view(-1)].view(N, N, -1).permute(2, 0, 1))  # (heads, query, key), float64
    table = P.swinv2_bias_table(mine, w["0.weight"], w["0.bias"], w["2.weight"])
    assert table.dtype == torch.float32 and table.shape == (heads, (2 * window - 1) ** 2)
    ty, tx = np.divmod(np.arange(N), window)
    idx = torch.from_numpy((ty[:, None] - ty[None, :] + window - 1) * (2 * window - 1) + (tx[:, None] - tx[None, :] + window - 1))  # the kernels' index: (query - key)
    assert torch.equal(idx, att.relative_position_index)
    assert float((table.double()[:, idx] - want).abs().max()) <= 16 * 2.0 ** -24  # one rounding of a value below 16 to float32
    assert float(want.max() - want.min()) > 1.0  # the MLP has real weights: the table is no constant


def test_logit_scale_is_clamped_then_exponentiated():
    from sleap_nn_amd.architectures import pretrained as P

    ls = torch.tensor([math.log(10.0), math.log(100.0) + 0.5, -1.0, math.log(100.0)]).view(4, 1, 1)
    got = P.swinv2_logit_scale(ls)
    want = torch.clamp(ls.double(), max=math.log(1.0 / 0.01)).exp().view(-1)
    assert got.shape == (4,) and got.dtype == torch.float32 and float((got.double() - want).abs().max()) <= 100 * 2.0 ** -24
    assert abs(float(got[1]) - 100.0) < 1e-4 and abs(float(got[0]) - 10.0) < 1e-5
    drawn = SC.draw_tensor("x.blocks.1.attention.self.logit_scale", (4, 1, 1), 3)
    assert float(drawn.max()) > math.log(100.0)  # the fixtures do reach the clamp


# ---- parameter names and loading

@pytest.mark.parametrize("name", ["A", "B"])
def test_parameter_names_and_order_equal_the_installed_backbone(name, tmp_path):
    tr = pytest.importorskip("transformers")
    arch = arch_of(name)
    enc = tr.Swinv2Backbone(tr.Swinv2Config(**{k: v for k, v in arch.items() if k != "model_type"}))
    m = new_model(name, tmp_path)
    mine = [k for k in m.param_shapes if k.startswith(ENC + ".")]
    want = list(enc.state_dict())  # (parameters only: the coordinate table and the position index are non-persistent buffers)
    assert mine == [ENC + "." + k for k in want]
    for k, v in enc.state_dict().items():
        assert tuple(m.param_shapes[ENC + "." + k]) == tuple(v.shape), k
    assert set(m.buffers) == {"backbone.image_mean", "backbone.image_std"}


@pytest.mark.parametrize("name", ["A", "B"])
def test_program_and_state_dict_round_trip(name, tmp_path):
    from sleap_nn_amd import _lib as L

    m = new_model(name, tmp_path)
    sd = golden_state(name, tmp_path)
    assert set(m.state_dict()) == set(sd)
    m.load_state_dict(sd, strict=True)
    back = m.state_dict()
    for k, v in sd.items():  # the round trip returns the reference's tensors, not the derived ones
        assert torch.equal(back[k], v), k
    k0 = f"{ENC}.encoder.layers.1.blocks.1.attention.self.key.weight"
    with pytest.raises(RuntimeError, match="key.weight"):
        m.load_state_dict({k: v for k, v in sd.items() if k != k0}, strict=True)
    kinds = [o.kind for o in m.ops]
    c = SC.FIXTURES[name]
    assert kinds[0] == L.OP_PATCH_STEM and m.ops[0].flags & L.FLAG_PAD0_NORM and kinds.count(L.OP_WINDOW_ATTN_V2) == sum(c["depths"]) and L.OP_WINDOW_ATTN not in kinds
    res_ln = [o for o in m.ops if o.kind == L.OP_LAYERNORM and o.flags & L.FLAG_RESIDUAL]
    assert len(res_ln) == 2 * sum(c["depths"]) and all(o.src1 >= 0 and o.src1 != o.dst and o.flags & L.FLAG_NO_TRAIN and o.flags & L.FLAG_LN_EPS_1EM5 for o in res_ln)
    merges = [o for o in m.ops if o.kind == L.OP_PATCH_MERGE]
    assert len(merges) == 3 and all(o.flags & L.FLAG_NO_NORM and o.flags & L.FLAG_NO_TRAIN and o.weight is None for o in merges)
    assert all(o.flags & L.FLAG_NO_TRAIN for o in m.ops if o.kind == L.OP_WINDOW_ATTN_V2)
    assert m.backbone.middle_slot == m.backbone.labels[f"{ENC}.stage4"] and m.backbone.encoder_ops() == max(i for i, o in enumerate(m.backbone.ops) if (o.weight or "").startswith(ENC)) + 1
    assert not any(o.kind == L.OP_GELU for o in m.ops)  # folded into the intermediate GEMM's epilogue for inference
    g0 = m.generation
    m.load_state_dict(sd, strict=True)
    assert m._handle is None and m.generation == g0


def test_model_hands_the_library_derived_tensors(tmp_path):
    """``Model._compile`` passes ``derived_params`` in place of four parameters of each block; the state keeps the reference's."""
    from sleap_nn_amd.architectures import pretrained as P

    m = new_model("B", tmp_path)
    sd = golden_state("B", tmp_path)
    m.load_state_dict(sd, strict=True)
    d = m.backbone.derived_params(m._state, m.buffers)
    assert len(d) == 4 * sum(SC.FIXTURES["B"]["depths"]) and set(d) <= set(m.param_shapes)
    a = f"{ENC}.encoder.layers.1.blocks.1.attention.self"
    C, heads, w = 64, 2, 7
    assert torch.equal(d[a + ".query.weight"], torch.cat([sd[a + ".query.weight"], sd[a + ".key.weight"], sd[a + ".value.weight"]]))
    qb = d[a + ".query.bias"]
    assert qb.shape == (3 * C,) and torch.equal(qb[:C], sd[a + ".query.bias"]) and float(qb[C:2 * C].abs().max()) == 0.0 and torch.equal(qb[2 * C:], sd[a + ".value.bias"])
    mlp = a + ".continuous_position_bias_mlp"
    assert torch.equal(d[mlp + ".2.weight"], P.swinv2_bias_table(P.swinv2_coords_table(w, 6), sd[mlp + ".0.weight"], sd[mlp + ".0.bias"], sd[mlp + ".2.weight"]))
    assert d[mlp + ".2.weight"].shape == (heads, (2 * w - 1) ** 2) and d[a + ".logit_scale"].shape == (heads,)
    assert abs(float(d[a + ".logit_scale"].max()) - 100.0) < 1e-4  # block 1's clamped head
    assert torch.equal(m._state[a + ".query.weight"], sd[a + ".query.weight"])
    for op in m.ops:
        if op.kind == P.L.OP_WINDOW_ATTN_V2:
            assert op.weight in d and op.bias in d and op.weight2 in d
    # the last stage of fixture A shrinks to window 2, and the table follows the stage's window
    ma = new_model("A", tmp_path)
    da = ma.backbone.derived_params(golden_state("A", tmp_path), {})
    assert da[f"{ENC}.encoder.layers.3.blocks.0.attention.self.continuous_position_bias_mlp.2.weight"].shape == (8, 9)


# ---- restatement parity

@pytest.mark.parametrize("name", ["A", "B"])
def test_restatement_reproduces_the_reference(name, tmp_path):
    g, sd = golden(name), golden_state(name, tmp_path)
    img = torch.from_numpy(g["frames"])
    bb, arch = bb_of(name, "unused"), arch_of(name)
    col = {}
    bo = R.backbone_forward(sd, bb, arch, img.float() / 255.0, col)
    assert len(bo["feature_maps"]) == 5
    for i, f in enumerate(bo["feature_maps"]):
        assert rel(f, g[f"feat/{i}"]) <= 1e-5, i
    layers = [k[len("layer/"):] for k in g if k.startswith("layer/")]
    assert len(layers) == 3 * sum(SC.FIXTURES[name]["depths"]) + 3
    for k in layers:  # (stored for frame 1 only)
        assert rel(col[k][1:2], g["layer/" + k]) <= 1e-5, k
    n_dec = sum(1 for k in g if k.startswith("dec/"))
    assert n_dec == len(bo["outputs"]) == {"A": 3, "B": 2}[name]
    for i, o in enumerate(bo["outputs"]):
        assert int(g[f"dec_stride/{i}"]) == bo["strides"][i]
        assert rel(o, g[f"dec/{i}"]) <= 1e-5, i
    out = R.model_forward(sd, bb, arch, heads_of(name), "single_instance", img)
    assert rel(out[HEAD], g["head"]) <= 1e-5


def test_golden_sees_clamp_bias_mlp_mask_and_batch(tmp_path):
    """Without the clamp, with a flat bias table or with the mask added once the head moves; frame 1 is about 0.2 of frame 0's intensity."""
    g, sd = golden("A"), golden_state("A", tmp_path)
    img = torch.from_numpy(g["frames"])
    bb, arch = bb_of("A", "unused"), arch_of("A")
    flat = {k: (torch.zeros_like(v) if k.endswith("continuous_position_bias_mlp.2.weight") else v) for k, v in sd.items()}
    assert rel(R.model_forward(flat, bb, arch, heads_of("A"), "single_instance", img)[HEAD], g["head"]) > 1e-3
    capped = {k: (torch.clamp(v, max=math.log(100.0)) if k.endswith("logit_scale") else v) for k, v in sd.items()}
    assert rel(R.model_forward(capped, bb, arch, heads_of("A"), "single_instance", img)[HEAD], g["head"]) <= 1e-5  # clamping by hand changes nothing: the clamp is applied
    assert max(float(v.max()) for k, v in sd.items() if k.endswith("logit_scale")) > math.log(100.0)
    m = img.float().mean(dim=(1, 2, 3))
    assert 0.1 < float(m[1] / m[0]) < 0.35


@pytest.mark.parametrize("name", ["A", "B", "W8"])
def test_restatement_equals_transformers(name):
    tr = pytest.importorskip("transformers")
    c, arch = SC.FIXTURES[name], arch_of(name)
    enc = tr.Swinv2Backbone(tr.Swinv2Config(**{k: v for k, v in arch.items() if k != "model_type"}, out_features=["stem", "stage1", "stage2", "stage3", "stage4"])).eval()
    sd = {k: torch.from_numpy(v) for k, v in SC.draw_state({ENC + "." + k: tuple(v.shape) for k, v in enc.state_dict().items()}, c["seed"]).items()}
    enc.load_state_dict({k[len(ENC) + 1:]: v for k, v in sd.items()})
    H, W = c["frame"]
    x = torch.randn(2, 3, H, W, generator=torch.Generator().manual_seed(7))
    x[1] *= 0.2
    with torch.no_grad():
        want = enc(x).feature_maps
    got = R.encoder_forward(sd, arch, x)
    assert len(got) == len(want) == 5
    for a, b in zip(got, want):
        assert a.shape == b.shape and rel(a, b) <= 1e-5


# ---- refusals and the opt-in

def test_refusals_by_name(tmp_path):
    from sleap_nn_amd.architectures.model import get_backbone

    cases = (({"num_heads": [2, 2, 4, 8]}, "head dimension"), ({"window_size": 16, "image_size": 256}, "window"), ({"window_size": 12, "image_size": 192}, "window"),
             ({"use_absolute_embeddings": True}, "use_absolute_embeddings"), ({"hidden_act": "relu"}, "hidden_act"), ({"layer_norm_eps": 1e-12}, "layer_norm_eps"),
             ({"qkv_bias": False}, "qkv_bias"), ({"num_channels": 1}, "in_channels"), ({"image_size": 4, "window_size": 4}, "window"))
    for over, word in cases:
        with pytest.raises(NotImplementedError, match=word):
            get_backbone("pretrained", bb_of("A", hf_dir("A", tmp_path, **over)))
    with pytest.raises(NotImplementedError, match="3 stages"):
        get_backbone("pretrained", bb_of("A", hf_dir("A", tmp_path, depths=[2, 2, 2], num_heads=[1, 2, 4])))
    for name in ("microsoft/swinv2-base-patch4-window16-256", "microsoft/swinv2-base-patch4-window12to16-192to256-22kto1k-ft", "microsoft/swinv2-base-patch4-window12-192-22k"):
        with pytest.raises(NotImplementedError, match="window"):
            get_backbone("pretrained", bb_of("A", name))
    ok = hf_dir("A", tmp_path)
    with pytest.raises(NotImplementedError, match="encoder"):
        get_backbone("pretrained", {**bb_of("A", ok), "mode": "encoder"})
    with pytest.raises(NotImplementedError, match="out_indices"):
        get_backbone("pretrained", {**bb_of("A", ok), "out_indices": [1, 3]})
    assert get_backbone("pretrained", {**bb_of("A", hf_dir("A", tmp_path, layer_norm_eps=1e-6))}).layer_norm_eps == 1e-6


def test_without_the_opt_in_the_refusal_names_key_and_keywords(tmp_path):
    from sleap_nn_amd.architectures.model import get_backbone

    for model_name in (W8_256, hf_dir("A", tmp_path)):
        with pytest.raises(NotImplementedError, match="allow_swinv2") as e:
            get_backbone("pretrained", bb_of("A", model_name, allow=False))
        assert "pretrained_swinv2" in str(e.value) and "build_model" in str(e.value) and "from_model_paths" in str(e.value) and "pretrained.py" in str(e.value)
    with pytest.raises(NotImplementedError, match="pretrained.py"):  # the ResNet opt-in does not open this family
        get_backbone("pretrained", {**bb_of("A", W8_256, allow=False), "allow_resnet": True})


def test_the_three_spellings_of_the_opt_in(tmp_path):
    import inspect

    from sleap_nn_amd.architectures.model import get_backbone
    from sleap_nn_amd.inference.loaders import load_model_assets
    from sleap_nn_amd.inference.predictor import Predictor

    assert get_backbone("pretrained", bb_of("A", hf_dir("A", tmp_path))).family == "swinv2"  # the config key
    m0 = new_model("A", tmp_path)
    sd = golden_state("A", tmp_path)
    run = write_run_dir(tmp_path / "run_a", "A", sd)
    a = load_model_assets(run)
    assert "allow_swinv2" not in a.backbone_config  # the config as the yaml has it
    with pytest.raises(NotImplementedError, match="pretrained_swinv2"):
        a.build_model()
    with pytest.raises(NotImplementedError, match="pretrained_swinv2"):
        a.build_model(pretrained_resnet=True)
    m = a.build_model(pretrained_swinv2=True)
    assert m.is_swinv2 and not m.is_resnet and m.backbone.channels == [32, 64, 128, 256] and m.backbone.window_size == 4 and list(m.param_shapes) == list(m0.param_shapes)
    for k in (f"{ENC}.encoder.layers.2.blocks.1.attention.self.logit_scale", "backbone.image_std", f"head_layers.0.{HEAD}.0.weight"):
        assert torch.equal(m.state_dict()[k], sd[k])
    assert "pretrained_swinv2" in inspect.signature(Predictor.from_model_paths).parameters  # (the predictor itself needs a device: tests/test_gpu_pretrained_swinv2.py)


def test_training_is_refused_by_name(tmp_path):
    from sleap_nn_amd.training.module import TrainingModule

    m = new_model("B", tmp_path)
    for kw in ({}, {"allow_pretrained": True}):
        with pytest.raises(NotImplementedError, match="Swinv2"):
            m.train(True, **kw)
    for kw in ({}, {"pretrained_training": True}):
        with pytest.raises(NotImplementedError, match="Swinv2"):
            TrainingModule(m, **kw)
    with pytest.raises(NotImplementedError, match="Swinv2"):
        m.backbone.check_trainable()
    assert m.eval() is m


def test_abi_and_build_list():
    from sleap_nn_amd import _lib as L
    from sleap_nn_amd import build

    with open(os.path.join(ROOT, "include", "posehip.h")) as f:
        header = f.read()
    assert int(re.search(r"^#define\s+PH_VERSION\s+(\d+)", header, re.M).group(1)) >= 132
    assert "int ph_debug_window_attn_v2_run(" in header and "PH_OP_WINDOW_ATTN_V2 = 22" in header and "#define PH_FLAG_NO_NORM 1024" in header
    assert "swinv2_kernels.hip" in build.SOURCES and "ph_debug_window_attn_v2_run" in L.SIGNATURES
    assert (L.OP_WINDOW_ATTN_V2, L.FLAG_NO_NORM, L.SWINV2_KV_WINDOW_ATTN, L.SWINV2_KV_LAYERNORM_ADD, L.SWINV2_KV_MERGE_GATHER) == (22, 1024, 32, 33, 34)
