"""The ``pretrained`` (HuggingFace ConvNeXtV2) backbone without a GPU: tests/convnextv2_ref.py against the reference's own outputs
(tests/golden/pretrained_convnextv2*.npz, written by tools/gen_pretrained_golden.py) and against ``transformers`` where it is installed; the
program's parameter names and shapes against the reference's state dict; architecture resolution, refusals and loading a run directory.

The bar for the restatement is that of tests/test_swint_cpu.py: 1e-5 of each map's scale."""
import json
import os

import numpy as np
import pytest
import torch

from tests import convnextv2_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
RUN_DIR = os.path.join(GOLD, "ckpt_dirs", "tiny_pretrained_convnextv2_single_instance")
PARTS = ["a", "b", "c"]
CONFIGS = {
    "A": {"depths": [1, 1, 2, 1], "hidden_sizes": [16, 32, 48, 64], "output_stride": 2, "normalize": True, "filters_rate": 1.5},
    "B": {"depths": [2, 1, 1, 1], "hidden_sizes": [24, 40, 48, 64], "output_stride": 4, "normalize": False, "filters_rate": 1.0},
}


def bb_of(name, model_name):
    c = CONFIGS[name]
    return {"source": "hf", "model_name": model_name, "in_channels": 3, "output_stride": c["output_stride"], "max_stride": 32, "weights": False, "mode": "decoder",
            "out_indices": None, "freeze": False, "revision": None, "normalize": c["normalize"], "image_mean": None, "image_std": None,
            "filters_rate": c["filters_rate"], "convs_per_block": 2, "kernel_size": 3, "up_interpolate": True}


def heads_of(name):
    return {"confmaps": {"part_names": PARTS, "sigma": 2.5, "output_stride": CONFIGS[name]["output_stride"], "loss_weight": 1.0}}


def hf_dir(name, tmp_path):
    """A directory with the configuration's ``config.json`` (A: the fixture's; B: written here -- settings only)."""
    if name == "A":
        return os.path.join(RUN_DIR, "hf_config")
    d = tmp_path / "hf_b"
    d.mkdir(exist_ok=True)
    c = CONFIGS[name]
    with open(d / "config.json", "w") as f:
        json.dump({"model_type": "convnextv2", "depths": c["depths"], "hidden_sizes": c["hidden_sizes"], "patch_size": 4, "num_channels": 3, "hidden_act": "gelu",
                   "layer_norm_eps": 1e-12}, f)
    return str(d)


_CACHE = {}


def golden(name):
    """(outputs npz as a dict, state dict) of a configuration, loaded once."""
    if name not in _CACHE:
        from sleap_nn_amd.inference.loaders import load_lightning_state_dict

        z = np.load(os.path.join(GOLD, "pretrained_convnextv2.npz" if name == "A" else "pretrained_convnextv2_b.npz"))
        g = {k: z[k] for k in z.files}
        if name == "A":
            sd = {k[len("model."):]: v for k, v in load_lightning_state_dict(os.path.join(RUN_DIR, "best.ckpt")).items()}
        else:
            s = np.load(os.path.join(GOLD, "pretrained_convnextv2_b_state.npz"))
            sd = {k: torch.from_numpy(s[k]) for k in s.files}
        _CACHE[name] = (g, sd)
    return _CACHE[name]


def rel(got, want):
    want = torch.as_tensor(want)
    return (torch.as_tensor(got) - want).abs().max().item() / max(1e-30, want.abs().max().item())


@pytest.mark.parametrize("name", ["A", "B"])
def test_restatement_reproduces_the_reference(name):
    """Every feature map (the dropped stem map included), every decoder output and the head output of the reference, to 1e-5 of each map's scale."""
    g, sd = golden(name)
    img = torch.from_numpy(g["frames"])
    bb = bb_of(name, "unused")
    bo = R.backbone_forward(sd, bb, img.float() / 255.0)
    assert len(bo["feature_maps"]) == 5
    for i, f in enumerate(bo["feature_maps"]):
        assert rel(f, g[f"feat/{i}"]) <= 1e-5, i
    n_dec = sum(1 for k in g if k.startswith("dec/"))
    assert n_dec == len(bo["outputs"]) == {"A": 4, "B": 3}[name]
    for i, o in enumerate(bo["outputs"]):
        assert int(g[f"dec_stride/{i}"]) == bo["strides"][i]
        assert rel(o, g[f"dec/{i}"]) <= 1e-5, i
    out = R.model_forward(sd, bb, heads_of(name), "single_instance", img)
    assert rel(out["SingleInstanceConfmapsHead"], g["head"]) <= 1e-5


def test_golden_sees_grn_and_the_batch():
    """With GRN's parameters zeroed the maps change (so a missing GRN fails the parity tests), and frame 1 is about 0.2 of the others' intensity."""
    g, sd = golden("A")
    assert all(float(sd[k].abs().max()) > 0.1 for k in sd if ".grn." in k)
    z = {k: (torch.zeros_like(v) if ".grn." in k else v) for k, v in sd.items()}
    img = torch.from_numpy(g["frames"])
    out = R.model_forward(z, bb_of("A", "unused"), heads_of("A"), "single_instance", img)["SingleInstanceConfmapsHead"]
    assert rel(out, g["head"]) > 1e-2
    m = img.float().mean(dim=(1, 2, 3))
    assert 0.1 < float(m[1] / m[0]) < 0.35 and 0.1 < float(m[1] / m[2]) < 0.35


def test_restatement_equals_transformers():
    """Directly against HuggingFace's ConvNextV2Backbone (all five maps), GRN parameters and norm affines re-drawn."""
    tr = pytest.importorskip("transformers")
    cfg = tr.ConvNextV2Config(num_channels=3, patch_size=4, num_stages=4, hidden_sizes=[24, 40, 48, 64], depths=[2, 1, 1, 1], hidden_act="gelu",
                              out_indices=[0, 1, 2, 3, 4])
    torch.manual_seed(5)
    enc = tr.ConvNextV2Backbone(cfg).eval()
    g = torch.Generator().manual_seed(6)
    with torch.no_grad():
        for n, p in enc.named_parameters():
            if ".grn." in n or "norm" in n or ".downsampling_layer.0." in n:
                p.copy_((1.0 if ("grn" not in n and n.endswith(".weight")) else 0.0) + 0.5 * torch.randn(p.shape, generator=g))
    x = torch.randn(3, 3, 64, 96, generator=g)
    x[1] *= 0.2
    with torch.no_grad():
        want = enc(x).feature_maps
    sd = {"backbone.enc." + k: v.detach() for k, v in enc.state_dict().items()}
    got = R.encoder_forward(sd, x)
    assert len(got) == len(want) == 5
    for a, b in zip(got, want):
        assert a.shape == b.shape and rel(a, b) <= 1e-5


@pytest.mark.parametrize("name", ["A", "B"])
def test_program_has_the_reference_state_dict(name, tmp_path):
    """``get_backbone("pretrained", ...)`` + heads: exactly the key set and shapes of the reference ``Model``'s state dict, buffers included; it loads strictly, the
    checkpoint's image statistics are the ones kept, and the unused stem norm loads too."""
    from sleap_nn_amd.architectures.model import Model, get_backbone

    _g, sd = golden(name)
    bb = bb_of(name, hf_dir(name, tmp_path))
    bbn = get_backbone("pretrained", bb)
    assert bbn.channels == CONFIGS[name]["hidden_sizes"] and bbn.depths == CONFIGS[name]["depths"] and bbn.max_stride == 32
    assert bbn.max_channels == 64 and bbn.middle_slot == bbn.labels["backbone.enc.hidden_states_norms.stage4"]
    m = Model("pretrained", bb, heads_of(name), "single_instance")
    mine = m.state_dict()
    assert set(mine) == set(sd)
    for k, v in sd.items():
        assert tuple(mine[k].shape) == tuple(v.shape), k
    assert tuple(mine["backbone.enc.encoder.stages.0.layers.0.grn.weight"].shape) == (1, 1, 1, 4 * CONFIGS[name]["hidden_sizes"][0])
    assert "backbone.enc.hidden_states_norms.stem.weight" in m.param_shapes
    assert not any(o.weight and "hidden_states_norms.stem" in o.weight for o in m.ops)
    other = dict(sd)
    other["backbone.image_mean"] = torch.tensor([0.1, 0.2, 0.3]).view(1, 3, 1, 1)
    m.load_state_dict(other, strict=True)
    assert torch.equal(m.state_dict()["backbone.image_mean"], other["backbone.image_mean"])
    assert torch.equal(m.state_dict()["backbone.enc.hidden_states_norms.stem.bias"], sd["backbone.enc.hidden_states_norms.stem.bias"])
    want_mean = [0.485, 0.456, 0.406] if CONFIGS[name]["normalize"] else [0.0, 0.0, 0.0]
    assert np.allclose(sd["backbone.image_mean"].reshape(-1).numpy(), want_mean)
    with pytest.raises(RuntimeError):
        m.load_state_dict({k: v for k, v in sd.items() if k != "backbone.image_std"}, strict=True)


def test_program_structure():
    """Every block carries a GRN between its GELU and its residual Linear; the GRN and stem ops are inference-only; the decoder's last block has no skip."""
    from sleap_nn_amd import _lib as L
    from sleap_nn_amd.architectures.model import Model

    m = Model("pretrained", bb_of("A", os.path.join(RUN_DIR, "hf_config")), heads_of("A"), "single_instance")
    kinds = [o.kind for o in m.unfused_ops]
    assert kinds.count(L.OP_GRN) == sum(CONFIGS["A"]["depths"])
    for i, o in enumerate(m.unfused_ops):
        if o.kind == L.OP_GRN:
            assert m.unfused_ops[i - 1].kind == L.OP_GELU and m.unfused_ops[i + 1].kind == L.OP_LINEAR and m.unfused_ops[i + 1].flags & L.FLAG_RESIDUAL
            assert o.flags & L.FLAG_NO_TRAIN
    assert m.unfused_ops[0].kind == L.OP_PATCH_STEM and m.unfused_ops[0].flags & L.FLAG_PAD0_NORM and m.unfused_ops[0].flags & L.FLAG_NO_TRAIN
    assert L.OP_GELU not in [o.kind for o in m.fused_ops] and L.OP_POOL not in kinds  # GELU rides in the first Linear; no additional pool, no middle blocks
    last = [o for o in m.unfused_ops if o.kind == L.OP_CONV and "_s4_to_s2_" in o.label]
    assert len(last) == 1 and last[0].src1 < 0
    assert m.backbone.decoder_stride_to_filters == {32: 64, 16: 36, 8: 24, 4: 16, 2: 16}


def test_size_table_and_local_directory(tmp_path, monkeypatch):
    from sleap_nn_amd.architectures import pretrained as P

    want = {"atto": ([2, 2, 6, 2], [40, 80, 160, 320]), "femto": ([2, 2, 6, 2], [48, 96, 192, 384]), "pico": ([2, 2, 6, 2], [64, 128, 256, 512]),
            "nano": ([2, 2, 8, 2], [80, 160, 320, 640]), "tiny": ([3, 3, 9, 3], [96, 192, 384, 768]), "base": ([3, 3, 27, 3], [128, 256, 512, 1024]),
            "large": ([3, 3, 27, 3], [192, 384, 768, 1536]), "huge": ([3, 3, 27, 3], [352, 704, 1408, 2816])}
    for size, (d, h) in want.items():
        a = P.resolve_architecture(f"facebook/convnextv2-{size}-22k-224")
        assert (a["depths"], a["hidden_sizes"], a["patch_size"]) == (d, h, 4)
    bbn = P.PretrainedBackbone.from_config({"output_stride": 4})  # the reference's default model_name: nano
    assert bbn.model_name == "facebook/convnextv2-nano-22k-224" and bbn.channels == [80, 160, 320, 640] and bbn.in_channels == 3
    # a relative name: the run directory first, then the working directory; a local config wins over a size word in the name
    run = tmp_path / "run"
    (run / "convnextv2-tiny-local").mkdir(parents=True)
    with open(run / "convnextv2-tiny-local" / "config.json", "w") as f:
        json.dump({"model_type": "convnextv2", "depths": [1, 1, 1, 1], "hidden_sizes": [16, 32, 48, 64], "patch_size": 4, "num_channels": 3, "hidden_act": "gelu"}, f)
    assert P.resolve_architecture("convnextv2-tiny-local", str(run))["hidden_sizes"] == [16, 32, 48, 64]
    assert P.resolve_architecture("convnextv2-tiny-local")["hidden_sizes"] == [96, 192, 384, 768]
    monkeypatch.chdir(run)
    assert P.resolve_architecture("convnextv2-tiny-local")["hidden_sizes"] == [16, 32, 48, 64]
    assert P.resolve_architecture(str(run / "convnextv2-tiny-local"))["depths"] == [1, 1, 1, 1]


def test_refusals(tmp_path):
    from sleap_nn_amd.architectures.model import Model, get_backbone

    for name in ("microsoft/resnet-50", "microsoft/swinv2-tiny-patch4-window8-256", "facebook/dinov2-with-registers-base", "facebook/dinov3-convnext-tiny-pretrain-lvd1689m"):
        with pytest.raises(NotImplementedError, match="pretrained.py"):
            get_backbone("pretrained", {"model_name": name, "output_stride": 4})
    d = tmp_path / "resnet"
    d.mkdir()
    with open(d / "config.json", "w") as f:
        json.dump({"model_type": "resnet", "depths": [3, 4, 6, 3], "hidden_sizes": [256, 512, 1024, 2048]}, f)
    with pytest.raises(NotImplementedError, match="resnet"):
        get_backbone("pretrained", {"model_name": str(d), "output_stride": 4})
    ok = "facebook/convnextv2-atto-1k-224"
    with pytest.raises(NotImplementedError, match="encoder"):
        get_backbone("pretrained", {"model_name": ok, "mode": "encoder", "output_stride": 4})
    with pytest.raises(NotImplementedError, match="out_indices"):
        get_backbone("pretrained", {"model_name": ok, "out_indices": [1, 3], "output_stride": 4})
    with pytest.raises(ValueError):
        get_backbone("pretrained", {"model_name": ok, "kernel_size": 5, "output_stride": 4})
    m = Model("pretrained", {"model_name": ok, "output_stride": 4, "freeze": True, "revision": "abc", "weights": True}, {"confmaps": {"part_names": PARTS, "sigma": 2.5, "output_stride": 4}},
              "single_instance")
    with pytest.raises(NotImplementedError, match="pretrained"):
        m.train()
    from sleap_nn_amd.training.module import TrainingModule

    with pytest.raises(NotImplementedError, match="pretrained"):
        TrainingModule(m)


def test_run_directory_loads():
    """best.ckpt + training_config.yaml whose ``model_name: hf_config`` is a directory next to the checkpoint (rule a)."""
    from sleap_nn_amd.inference.loaders import load_model_assets

    a = load_model_assets(RUN_DIR)
    assert a.backbone_type == "pretrained" and a.model_type == "single_instance" and a.backbone_config["model_name"] == "hf_config"
    assert set(a.backbone_config) == set(bb_of("A", "x"))  # the config as the yaml has it: nothing of this host is added to it
    m = a.build_model()
    assert m.backbone.channels == [16, 32, 48, 64] and m.backbone.depths == [1, 1, 2, 1] and m.in_channels == 3
    _g, sd = golden("A")
    for k in ("backbone.enc.encoder.stages.2.layers.1.grn.weight", "backbone.image_std", "head_layers.0.SingleInstanceConfmapsHead.0.weight"):
        assert torch.equal(m.state_dict()[k], sd[k])


NODES = ["a", "b", "c"]
EDGES = [["a", "b"], ["b", "c"]]
CM = {"part_names": NODES, "sigma": 2.5, "output_stride": 4, "loss_weight": 1.0, "anchor_part": None}
HEAD_CONFIGS = {
    "single_instance": {"confmaps": CM},
    "centroid": {"confmaps": {"anchor_part": None, "sigma": 2.5, "output_stride": 4, "loss_weight": 1.0}},
    "centered_instance": {"confmaps": CM},
    "bottomup": {"confmaps": CM, "pafs": {"edges": EDGES, "sigma": 15.0, "output_stride": 8, "loss_weight": 1.0}},
    "multi_class_bottomup": {"confmaps": CM, "class_maps": {"classes": ["x", "y"], "sigma": 5.0, "output_stride": 8, "loss_weight": 1.0}},
    "multi_class_topdown": {"confmaps": CM, "class_vectors": {"classes": ["x", "y"], "num_fc_layers": 1, "num_fc_units": 16, "global_pool": True, "output_stride": 32, "loss_weight": 1.0}},
}


@pytest.mark.parametrize("model_type", sorted(HEAD_CONFIGS))
def test_every_pose_model_type_builds(model_type):
    """The model types a ConvNeXt backbone carries build on this one; the class-vector head sits on the bottleneck (the normed stage-4 map, 320 channels at atto)."""
    from sleap_nn_amd import _lib as L
    from sleap_nn_amd.architectures.model import Model

    m = Model("pretrained", {"model_name": "facebook/convnextv2-atto-1k-224", "output_stride": 4}, HEAD_CONFIGS[model_type], model_type)
    heads = [o for o in m.ops if o.kind == L.OP_HEAD]
    assert len(heads) == len(m.heads) and set(m.state_dict()) >= {"backbone.image_mean", "backbone.image_std"}
    if model_type == "multi_class_topdown":
        pool = next(o for o in m.ops if o.kind == L.OP_GLOBAL_MAXPOOL)
        assert pool.src0 == m.backbone.middle_slot and pool.cin0 == 320
