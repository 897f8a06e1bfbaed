"""Generate the goldens of the ``pretrained`` (HuggingFace ConvNeXtV2) backbone from the reference's own code, where the reference tree and
``transformers`` are available (CPU only, no network: the HuggingFace config is written to a local directory and the model is built with
``weights=False``):

* ``tests/golden/pretrained_convnextv2.npz`` (configuration A) and ``pretrained_convnextv2_b.npz`` (B): the uint8 frames, every encoder feature
  map (``feat/<i>``: stem, stage1..4), every decoder output (``dec/<i>``), the head output and the oracle's single-instance peaks on it;
  ``pretrained_convnextv2_b_state.npz``: B's state dict (A's is the run directory's checkpoint).  One file each, to stay under the size limit
  of a committed file;
* ``tests/golden/ckpt_dirs/tiny_pretrained_convnextv2_single_instance``: ``best.ckpt`` + ``training_config.yaml`` + ``hf_config/config.json`` of
  configuration A (the yaml names the architecture as ``model_name: hf_config``, a directory next to the checkpoint).

``transformers`` is imported BEFORE ``oracle.ref_harness.install()``: the harness's torchvision stand-in breaks a later ``import transformers``.
HuggingFace initialises GRN's weight and bias to zeros, which makes GRN the identity: every GRN parameter and every norm affine is re-drawn, so
that a missing or wrong GRN changes the golden.  The reference runs in ``eval()``.

    python tools/gen_pretrained_golden.py
"""
import os
import sys
import types

import numpy as np
import torch
import yaml

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GOLD = os.path.join(ROOT, "tests", "golden")
RUN_DIR = os.path.join(GOLD, "ckpt_dirs", "tiny_pretrained_convnextv2_single_instance")
B, H, W = 3, 64, 96
PARTS = ["a", "b", "c"]

CONFIGS = {
    "A": {"depths": [1, 1, 2, 1], "hidden_sizes": [16, 32, 48, 64], "output_stride": 2, "normalize": True, "filters_rate": 1.5, "seed": 101},
    # widths that are no multiples of 16: pad channels in every stage-1 / stage-2 tensor; the hidden 4C widths stay whole
    "B": {"depths": [2, 1, 1, 1], "hidden_sizes": [24, 40, 48, 64], "output_stride": 4, "normalize": False, "filters_rate": 1.0, "seed": 202},
}


def backbone_config(name, model_name):
    c = CONFIGS[name]
    return {"source": "hf", "model_name": model_name, "in_channels": 3, "output_stride": c["output_stride"], "max_stride": 32, "weights": False, "mode": "decoder",
            "out_indices": None, "freeze": False, "revision": None, "normalize": c["normalize"], "image_mean": None, "image_std": None, "filters_rate": c["filters_rate"],
            "convs_per_block": 2, "kernel_size": 3, "up_interpolate": True}


def head_config(name):
    return {"confmaps": {"part_names": PARTS, "sigma": 2.5, "output_stride": CONFIGS[name]["output_stride"], "loss_weight": 1.0}}


def frames(seed):
    """Blobs on noise, three channels; frame 1 at about 0.2 of the others' intensity (a reduction that wrongly spans the batch then changes the answer)."""
    g = np.random.default_rng(seed)
    fr = 40.0 + 25.0 * g.standard_normal((B, 3, H, W))
    yy, xx = np.mgrid[0:H, 0:W]
    for b in range(B):
        for _ in range(4):
            cx, cy, s = g.uniform(8, W - 8), g.uniform(8, H - 8), g.uniform(3.0, 6.0)
            fr[b] += g.uniform(80, 200, size=(3, 1, 1)) * np.exp(-((xx - cx) ** 2 + (yy - cy) ** 2) / (2 * s * s))
    fr[1] *= 0.2
    return np.clip(fr, 0, 255).astype(np.uint8)


def build(name, hf_dir, seed):
    import transformers  # noqa: F401  (first: see the module docstring)
    from transformers import ConvNextV2Config

    from oracle import ref_harness as rh

    c = CONFIGS[name]
    os.makedirs(hf_dir, exist_ok=True)
    ConvNextV2Config(num_channels=3, patch_size=4, num_stages=4, hidden_sizes=c["hidden_sizes"], depths=c["depths"], hidden_act="gelu").save_pretrained(hf_dir)
    rh.install()
    if "lightning" not in sys.modules:
        lm = types.ModuleType("lightning")
        lm.LightningModule = torch.nn.Module
        sys.modules["lightning"] = lm
    import sleap_nn.architectures.pretrained as rp

    if not hasattr(rp.OmegaConf, "select"):  # the harness's stand-in lacks it; PretrainedBackbone.from_config reads its leaf through it
        def select(cfg, key, default=None):
            try:
                v = cfg[key]
            except (KeyError, AttributeError, TypeError):
                return default
            return default if v is None else v

        rp.OmegaConf = types.SimpleNamespace(select=select)
    from sleap_nn.architectures.model import Model

    torch.manual_seed(seed)
    bb = backbone_config(name, hf_dir)
    m = Model("pretrained", rh.attrdict(bb), rh.attrdict(head_config(name)), "single_instance").eval()
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for n, p in m.named_parameters():
            is_norm = "norm" in n or ".downsampling_layer.0." in n  # embeddings.layernorm, layers.*.layernorm, downsampling_layer.0, hidden_states_norms.*
            if ".grn." in n:
                p.copy_(0.5 * torch.randn(p.shape, generator=g))
            elif is_norm:
                p.copy_((1.0 if n.endswith(".weight") else 0.0) + 0.5 * torch.randn(p.shape, generator=g))
            elif p.dim() > 1:
                torch.nn.init.xavier_uniform_(p, generator=g)
            else:
                p.copy_(0.2 * (torch.rand(p.shape, generator=g) * 2 - 1))
    return m.eval(), bb


def run(name, m, img):
    from oracle import cpu_ref as O

    out = {}
    x = torch.from_numpy(img).float() / 255.0
    with torch.no_grad():
        bbm = m.backbone
        feats = bbm.enc(bbm._normalize(x)).feature_maps
        res = bbm(x)
        heads = m(x)
    assert len(feats) == 5 and not bbm.enc.training
    for i, f in enumerate(feats):
        out[f"feat/{i}"] = f.numpy()
    for i, (s, o) in enumerate(zip(res["strides"], res["outputs"])):
        out[f"dec/{i}"] = o.numpy()
        out[f"dec_stride/{i}"] = np.int64(s)
    assert list(heads) == ["SingleInstanceConfmapsHead"]
    cms = heads["SingleInstanceConfmapsHead"]
    out[f"head"] = cms.numpy()
    thr = float(cms.amax(dim=(2, 3)).min()) - 0.05 * max(1.0, float(cms.abs().max()))  # below every map's maximum, with room
    pk, pv = O.single_instance_postprocess(cms, CONFIGS[name]["output_stride"], peak_threshold=thr)[:2]
    pk, pv = np.asarray(pk), np.asarray(pv)
    assert not np.isnan(pk).any(), "every part must give a peak"
    scale = max(1.0, float(cms.abs().max()))
    for b in range(cms.shape[0]):  # the arg max must be clear of the runner-up outside its 5 x 5 neighbourhood, or 1e-4 of noise could move the peak
        for c in range(cms.shape[1]):
            mp = cms[b, c].clone()
            iy, ix = np.unravel_index(int(mp.argmax()), mp.shape)
            top = float(mp[iy, ix])
            mp[max(0, iy - 2): iy + 3, max(0, ix - 2): ix + 3] = -1e30
            assert top - float(mp.max()) > 2e-3 * scale, (name, b, c, top - float(mp.max()))
    out[f"peaks"], out[f"peak_vals"], out[f"peak_threshold"] = pk.astype(np.float32), pv.astype(np.float32), np.float32(thr)
    out[f"frames"] = img
    return out


def training_config(name):
    heads = {k: None for k in ("single_instance", "centroid", "centered_instance", "bottomup", "multi_class_bottomup", "multi_class_topdown",
                               "bottomup_segmentation", "semantic_segmentation", "centered_instance_segmentation")}
    heads["single_instance"] = head_config(name)
    pre = {"ensure_rgb": True, "ensure_grayscale": False, "max_height": None, "max_width": None, "scale": 1.0, "crop_size": None}
    skel = {"name": "s", "nodes": [{"name": n} for n in PARTS], "edges": []}
    return {"data_config": {"preprocessing": pre, "skeletons": [skel]},
            "model_config": {"backbone_config": {"unet": None, "convnext": None, "swint": None, "pretrained": backbone_config(name, "hf_config")}, "head_configs": heads},
            "trainer_config": {"run_name": os.path.basename(RUN_DIR)}, "name": "", "description": "", "sleap_nn_version": "0.0.1"}


def main():
    import tempfile

    os.makedirs(RUN_DIR, exist_ok=True)
    written = []
    with tempfile.TemporaryDirectory() as tmp:
        for name in CONFIGS:
            hf_dir = os.path.join(RUN_DIR, "hf_config") if name == "A" else os.path.join(tmp, "hf_" + name)
            for attempt in range(20):  # the first weight seed whose peaks are clear of their runners-up (the margin asserted in run())
                m, _bb = build(name, hf_dir, CONFIGS[name]["seed"] + 1000 * attempt)
                try:
                    gold = run(name, m, frames(CONFIGS[name]["seed"]))
                    break
                except AssertionError as e:
                    print(f"{name}: weight seed +{1000 * attempt} rejected: {e}")
            else:
                raise RuntimeError("no seed gives clear peaks")
            path = os.path.join(GOLD, "pretrained_convnextv2.npz" if name == "A" else "pretrained_convnextv2_b.npz")
            np.savez_compressed(path, **gold)
            written.append(path)
            if name == "A":
                torch.save({"state_dict": {"model." + k: v.detach().clone() for k, v in m.state_dict().items()}}, os.path.join(RUN_DIR, "best.ckpt"))
                with open(os.path.join(RUN_DIR, "training_config.yaml"), "w") as f:
                    yaml.safe_dump(training_config(name), f, sort_keys=False)
                written.append(os.path.join(RUN_DIR, "best.ckpt"))
            else:
                path = os.path.join(GOLD, "pretrained_convnextv2_b_state.npz")
                np.savez_compressed(path, **{k: v.detach().numpy() for k, v in m.state_dict().items()})
                written.append(path)
    for p in written:
        assert os.path.getsize(p) < (1 << 20), p
        print(f"wrote {p} ({os.path.getsize(p) / 1024:.0f} KiB)")


if __name__ == "__main__":
    main()
