"""The ResNet family of the ``pretrained`` backbone without a GPU: architecture resolution and its refusals, the program's parameter and buffer names against
the reference's state dict, loading, the BatchNorm fold, and tests/resnet_ref.py against the reference's own outputs (tests/golden/pretrained_resnet*.npz,
written by tools/gen_pretrained_resnet_golden.py) and against ``transformers`` where it is installed.

The bar for the restatement is that of tests/test_pretrained_cpu.py: 1e-5 of each map's scale."""
import json
import os

import numpy as np
import pytest
import torch

from tests import resnet_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
RUN_DIR = os.path.join(GOLD, "ckpt_dirs", "tiny_pretrained_resnet_single_instance")
PARTS = ["a", "b", "c"]
CONFIGS = {
    "A": {"layer_type": "bottleneck", "embedding_size": 16, "hidden_sizes": [32, 64, 96, 128], "depths": [2, 1, 2, 1], "output_stride": 2, "normalize": True, "filters_rate": 1.5},
    "B": {"layer_type": "basic", "embedding_size": 24, "hidden_sizes": [24, 40, 48, 64], "depths": [2, 1, 1, 1], "output_stride": 4, "normalize": False, "filters_rate": 1.0},
}


def hf_json(c, **over):
    return {"model_type": "resnet", "embedding_size": c["embedding_size"], "hidden_sizes": c["hidden_sizes"], "depths": c["depths"], "layer_type": c["layer_type"],
            "hidden_act": "relu", "num_channels": 3, "downsample_in_first_stage": False, "downsample_in_bottleneck": False, **over}


def bb_of(name, model_name, allow=True):
    c = CONFIGS[name]
    bb = {"source": "hf", "model_name": model_name, "in_channels": 3, "output_stride": c["output_stride"], "max_stride": 32, "weights": False, "mode": "decoder",
          "out_indices": None, "freeze": False, "revision": None, "normalize": c["normalize"], "image_mean": None, "image_std": None,
          "filters_rate": c["filters_rate"], "convs_per_block": 2, "kernel_size": 3, "up_interpolate": True}
    if allow:
        bb["allow_resnet"] = True
    return bb


def heads_of(name):
    return {"confmaps": {"part_names": PARTS, "sigma": 2.5, "output_stride": CONFIGS[name]["output_stride"], "loss_weight": 1.0}}


def hf_dir(name, tmp_path, **over):
    """A directory with the configuration's ``config.json`` (A without overrides: the fixture's; else written here -- settings only)."""
    if name == "A" and not over:
        return os.path.join(RUN_DIR, "hf_config")
    d = tmp_path / ("hf_" + name + "_".join(sorted(over)))
    d.mkdir(exist_ok=True)
    with open(d / "config.json", "w") as f:
        json.dump(hf_json(CONFIGS[name], **over), f)
    return str(d)


_CACHE = {}


def golden(name):
    """(outputs npz + layer outputs as one dict, state dict in fp32) of a configuration, loaded once."""
    if name not in _CACHE:
        from sleap_nn_amd.inference.loaders import load_lightning_state_dict

        stem = "pretrained_resnet" if name == "A" else "pretrained_resnet_b"
        g = {}
        for f in (stem + ".npz", stem + "_layers.npz"):
            z = np.load(os.path.join(GOLD, f))
            g.update({k: z[k] for k in z.files})
        if name == "A":  # (the run directory's checkpoint holds fp16 tensors, every value fp16-exact: tools/gen_pretrained_resnet_golden.py)
            sd = {k[len("model."):]: (v.float() if v.is_floating_point() else v) for k, v in load_lightning_state_dict(os.path.join(RUN_DIR, "best.ckpt")).items()}
        else:
            s = np.load(os.path.join(GOLD, "pretrained_resnet_b_state.npz"))
            sd = {k: torch.from_numpy(s[k]) for k in s.files}
        _CACHE[name] = (g, sd)
    return _CACHE[name]


def rel(got, want):
    want = torch.as_tensor(want)
    return (torch.as_tensor(got) - want).abs().max().item() / max(1e-30, want.abs().max().item())


# ---- resolution

def test_resolution_from_config_json_and_table(tmp_path):
    from sleap_nn_amd.architectures import pretrained as P

    for name, c in CONFIGS.items():
        a = P.resolve_architecture(hf_dir(name, tmp_path), allow_resnet=True)
        assert a["family"] == "resnet" and a["patch_size"] == 4
        assert {k: a[k] for k in ("embedding_size", "hidden_sizes", "depths", "layer_type", "num_channels")} == {**{k: c[k] for k in ("embedding_size", "hidden_sizes", "depths", "layer_type")}, "num_channels": 3}
    want = {"18": ("basic", [2, 2, 2, 2], [64, 128, 256, 512]), "34": ("basic", [3, 4, 6, 3], [64, 128, 256, 512]), "26": ("bottleneck", [2, 2, 2, 2], [256, 512, 1024, 2048]),
            "50": ("bottleneck", [3, 4, 6, 3], [256, 512, 1024, 2048]), "101": ("bottleneck", [3, 4, 23, 3], [256, 512, 1024, 2048]), "152": ("bottleneck", [3, 8, 36, 3], [256, 512, 1024, 2048])}
    for n, (lt, d, h) in want.items():
        a = P.resolve_architecture(f"microsoft/resnet-{n}", allow_resnet=True)
        assert (a["family"], a["layer_type"], a["depths"], a["hidden_sizes"], a["embedding_size"], a["num_channels"]) == ("resnet", lt, d, h, 64, 3)
    bbn = P.PretrainedBackbone.from_config({"model_name": "microsoft/resnet-18", "output_stride": 4, "allow_resnet": True})
    assert bbn.family == "resnet" and bbn.channels == [64, 128, 256, 512] and bbn.max_stride == 32 and bbn.max_channels == 512
    assert P.resolve_architecture("facebook/convnextv2-atto-1k-224", allow_resnet=True)["family"] == "convnextv2"  # the opt-in changes nothing else


def test_resnet50_row_is_the_installed_default():
    tr = pytest.importorskip("transformers")
    from sleap_nn_amd.architectures import pretrained as P

    c = tr.ResNetConfig()
    a = P.resolve_architecture("microsoft/resnet-50", allow_resnet=True)
    assert (a["embedding_size"], a["hidden_sizes"], a["depths"], a["layer_type"]) == (c.embedding_size, list(c.hidden_sizes), list(c.depths), c.layer_type)
    assert c.hidden_act == "relu" and not c.downsample_in_first_stage and not c.downsample_in_bottleneck and c.num_channels == 3


def test_refusals_by_name(tmp_path):
    from sleap_nn_amd.architectures.model import get_backbone

    for over, word in (({"downsample_in_first_stage": True}, "downsample_in_first_stage"), ({"downsample_in_bottleneck": True}, "downsample_in_bottleneck"),
                       ({"hidden_act": "gelu"}, "hidden_act"), ({"num_channels": 1}, "in_channels")):
        with pytest.raises(NotImplementedError, match=word):
            get_backbone("pretrained", bb_of("A", hf_dir("A", tmp_path, **over)))
    with pytest.raises(NotImplementedError, match="3 stages"):
        get_backbone("pretrained", bb_of("A", hf_dir("A", tmp_path, hidden_sizes=[32, 64, 96], depths=[1, 1, 1])))
    ok = hf_dir("A", tmp_path)
    with pytest.raises(NotImplementedError, match="encoder"):
        get_backbone("pretrained", {**bb_of("A", ok), "mode": "encoder"})
    with pytest.raises(NotImplementedError, match="out_indices"):
        get_backbone("pretrained", {**bb_of("A", ok), "out_indices": [1, 3]})


def test_without_the_opt_in_the_refusal_names_key_and_keyword(tmp_path):
    from sleap_nn_amd.architectures.model import get_backbone
    from sleap_nn_amd.inference.loaders import load_model_assets

    for model_name in ("microsoft/resnet-50", hf_dir("A", tmp_path)):
        with pytest.raises(NotImplementedError, match="allow_resnet") as e:
            get_backbone("pretrained", bb_of("A", model_name, allow=False))
        assert "pretrained_resnet" in str(e.value) and "pretrained.py" in str(e.value)
    a = load_model_assets(RUN_DIR)
    assert "allow_resnet" not in a.backbone_config  # the config as the yaml has it
    with pytest.raises(NotImplementedError, match="pretrained_resnet"):
        a.build_model()
    m = a.build_model(pretrained_resnet=True)
    assert m.is_resnet and m.backbone.channels == [32, 64, 96, 128] and m.backbone.layer_type == "bottleneck"
    _g, sd = golden("A")
    for k in ("backbone.enc.encoder.stages.2.layers.1.layer.1.normalization.running_var", "backbone.image_std", "head_layers.0.SingleInstanceConfmapsHead.0.weight"):
        assert torch.equal(m.state_dict()[k], sd[k])


# ---- parameter names and loading

@pytest.mark.parametrize("name", ["A", "B"])
def test_program_has_the_reference_state_dict(name, tmp_path):
    from sleap_nn_amd import _lib as L
    from sleap_nn_amd.architectures.model import Model

    _g, sd = golden(name)
    m = Model("pretrained", bb_of(name, hf_dir(name, tmp_path)), heads_of(name), "single_instance")
    mine = m.state_dict()
    assert set(mine) == set(sd)
    for k, v in sd.items():
        assert tuple(mine[k].shape) == tuple(v.shape), k
    fresh = [k for k in mine if k.endswith(".running_mean")]
    assert fresh and all(float(mine[k].abs().max()) == 0.0 and float((mine[k.replace("running_mean", "running_var")] - 1).abs().max()) == 0.0 for k in fresh)
    m.load_state_dict(sd, strict=True)
    back = m.state_dict()
    for k, v in sd.items():  # the round trip returns the UNFOLDED tensors (num_batches_tracked is accepted and ignored)
        if not k.endswith("num_batches_tracked"):
            assert torch.equal(back[k], v.float()), k
    rv = next(k for k in sd if k.endswith(".layer.1.normalization.running_var"))
    with pytest.raises(RuntimeError, match="running_var"):
        m.load_state_dict({k: v for k, v in sd.items() if k != rv}, strict=True)
    tracked = {k: (torch.tensor(7) if k.endswith("num_batches_tracked") else v) for k, v in sd.items()}
    m.load_state_dict(tracked, strict=True)
    # the program: no op reads a BatchNorm weight; the stem, the strided convs and (basic layers) the add are the new kinds; the pyramid is the raw stage outputs
    kinds = [o.kind for o in m.ops]
    assert kinds[0] == L.OP_RESNET_STEM and L.OP_LAYERNORM not in kinds and L.OP_CONV_S2 in kinds
    assert (L.OP_ADD_RELU in kinds) == (name == "B")
    assert not any((o.weight or "").endswith("normalization.weight") for o in m.ops)
    assert m.backbone.middle_slot == m.backbone.labels["backbone.enc.stage4"]
    first = "backbone.enc.encoder.stages.0.layers.0.shortcut.convolution.weight"
    assert (first in sd) == (name == "A")  # B: 24 -> 24 at stride 1 has no shortcut module
    g0 = m.generation
    m.load_state_dict(sd, strict=True)  # a handle (none here) would have been released: the fold never outlives its inputs
    assert m._handle is None and m.generation == g0


# ---- restatement parity

@pytest.mark.parametrize("name", ["A", "B"])
def test_restatement_reproduces_the_reference(name):
    g, sd = golden(name)
    img = torch.from_numpy(g["frames"])
    bb = bb_of(name, "unused")
    col = {}
    bo = R.backbone_forward(sd, bb, img.float() / 255.0, col)
    assert len(bo["feature_maps"]) == 5
    for i, f in enumerate(bo["feature_maps"]):
        assert rel(f, g[f"feat/{i}"]) <= 1e-5, i
    layers = [k[len("layer/"):] for k in g if k.startswith("layer/")]
    assert len(layers) >= 15
    for k in layers:
        assert rel(col[k], g["layer/" + k]) <= 1e-5, k
    n_dec = sum(1 for k in g if k.startswith("dec/"))
    assert n_dec == len(bo["outputs"]) == {"A": 4, "B": 3}[name]
    for i, o in enumerate(bo["outputs"]):
        assert int(g[f"dec_stride/{i}"]) == bo["strides"][i]
        assert rel(o, g[f"dec/{i}"]) <= 1e-5, i
    out = R.model_forward(sd, bb, heads_of(name), "single_instance", img)
    assert rel(out["SingleInstanceConfmapsHead"], g["head"]) <= 1e-5


def test_golden_sees_batchnorm_and_the_batch():
    """With BatchNorm at its initial values the maps change (a missing fold fails the parity tests), and frame 1 is about 0.2 of the others' intensity."""
    g, sd = golden("A")
    ident = {k: (torch.ones_like(v) if k.endswith("running_var") or k.endswith("normalization.weight") else torch.zeros_like(v)) if ".normalization." in k and v.is_floating_point() else v
             for k, v in sd.items()}
    img = torch.from_numpy(g["frames"])
    out = R.model_forward(ident, bb_of("A", "unused"), heads_of("A"), "single_instance", img)["SingleInstanceConfmapsHead"]
    assert rel(out, g["head"]) > 1e-2
    m = img.float().mean(dim=(1, 2, 3))
    assert 0.1 < float(m[1] / m[0]) < 0.35 and 0.1 < float(m[1] / m[2]) < 0.35


@pytest.mark.parametrize("layer_type", ["basic", "bottleneck"])
def test_restatement_equals_transformers(layer_type):
    tr = pytest.importorskip("transformers")
    cfg = tr.ResNetConfig(num_channels=3, embedding_size=24, hidden_sizes=[24, 40, 48, 64], depths=[2, 1, 2, 1], layer_type=layer_type, hidden_act="relu",
                          out_indices=[0, 1, 2, 3, 4])
    torch.manual_seed(5)
    enc = tr.ResNetBackbone(cfg).eval()
    sd = R.draw_batchnorm_({"backbone.enc." + k: v.detach().clone() for k, v in enc.state_dict().items()}, torch.Generator().manual_seed(6))
    enc.load_state_dict({k[len("backbone.enc."):]: v for k, v in sd.items()})
    x = torch.randn(3, 3, 64, 96, generator=torch.Generator().manual_seed(7))
    x[1] *= 0.2
    with torch.no_grad():
        want = enc(x).feature_maps
    got = R.encoder_forward(sd, x)
    assert len(got) == len(want) == 5
    for a, b in zip(got, want):
        assert a.shape == b.shape and rel(a, b) <= 1e-5


# ---- fold

@pytest.mark.parametrize("k,stride", [(1, 1), (3, 1), (3, 2), (7, 2)])
def test_fold_equals_batchnorm_in_float64(k, stride):
    """conv -> BatchNorm (eval) against the folded conv + bias, both evaluated in float64: the fold is exact arithmetic, so they agree to float32 rounding of the folded tensors."""
    import torch.nn.functional as F

    from sleap_nn_amd.architectures.pretrained import BN_EPS, fold_batchnorm

    g = torch.Generator().manual_seed(k * 10 + stride)
    w = torch.randn(10, 6, k, k, generator=g)
    gamma, beta, mean, var = 1 + 0.3 * torch.randn(10, generator=g), 0.3 * torch.randn(10, generator=g), 0.3 * torch.randn(10, generator=g), 0.5 + 1.5 * torch.rand(10, generator=g)
    x = torch.randn(2, 6, 12, 14, generator=g).double()
    want = F.batch_norm(F.conv2d(x, w.double(), None, stride=stride, padding=k // 2), mean.double(), var.double(), gamma.double(), beta.double(), False, 0.0, BN_EPS)
    wf, bf = fold_batchnorm(w, gamma, beta, mean, var)
    assert wf.dtype == torch.float32 and bf.dtype == torch.float32 and wf.shape == w.shape and bf.shape == (10,)
    got = F.conv2d(x, wf.double(), bf.double(), stride=stride, padding=k // 2)
    assert rel(got, want) <= 4 * 2.0 ** -24  # one rounding of each folded value to float32 (2^-24 relative each), a few of them per output
    # the order matters: folding with mean and beta swapped is far off
    wf2, bf2 = fold_batchnorm(w, gamma, mean, beta, var)
    assert rel(F.conv2d(x, wf2.double(), bf2.double(), stride=stride, padding=k // 2), want) > 1e-2


def test_model_hands_the_library_folded_tensors(tmp_path):
    """``Model._compile`` passes ``folded_params`` in place of the conv weight and the BatchNorm bias; the state keeps the unfolded ones."""
    from sleap_nn_amd.architectures.model import Model
    from sleap_nn_amd.architectures.pretrained import fold_batchnorm

    _g, sd = golden("B")
    m = Model("pretrained", bb_of("B", hf_dir("B", tmp_path)), heads_of("B"), "single_instance")
    m.load_state_dict(sd, strict=True)
    f = m.backbone.folded_params(m._state, m.buffers)
    assert len(f) == 2 * len(m.backbone.bn_convs) and set(f) <= set(m.param_shapes)
    n = "backbone.enc.encoder.stages.1.layers.0.shortcut"
    wf, bf = fold_batchnorm(sd[n + ".convolution.weight"], sd[n + ".normalization.weight"], sd[n + ".normalization.bias"], sd[n + ".normalization.running_mean"],
                            sd[n + ".normalization.running_var"])
    assert torch.equal(f[n + ".convolution.weight"], wf) and torch.equal(f[n + ".normalization.bias"], bf)
    assert torch.equal(m._state[n + ".convolution.weight"], sd[n + ".convolution.weight"])
    for op in m.ops:  # every encoder conv reads exactly one folded pair
        if (op.weight or "").startswith("backbone.enc."):
            assert op.weight in f and op.bias in f and op.bias == op.weight.replace("convolution.weight", "normalization.bias")


def test_training_is_refused_by_name(tmp_path):
    from sleap_nn_amd.architectures.model import Model
    from sleap_nn_amd.training.module import TrainingModule

    m = Model("pretrained", bb_of("B", hf_dir("B", tmp_path)), heads_of("B"), "single_instance")
    for kw in ({}, {"allow_pretrained": True}):
        with pytest.raises(NotImplementedError, match="ResNet"):
            m.train(True, **kw)
    for kw in ({}, {"pretrained_training": True}):
        with pytest.raises(NotImplementedError, match="ResNet"):
            TrainingModule(m, **kw)
    assert m.eval() is m
