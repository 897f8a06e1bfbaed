"""Generate the goldens of the ``pretrained`` backbone's ResNet family (HuggingFace ``ResNetBackbone``) from the reference's own code, where the
reference tree and ``transformers`` are available (CPU only, no network), on the pattern of tools/gen_pretrained_golden.py:

* ``tests/golden/pretrained_resnet.npz`` (configuration A, bottleneck layers) and ``pretrained_resnet_b.npz`` (B, basic layers): the uint8 frames, the
  five encoder feature maps (``feat/<i>``: stem, stage1..4), the output of every conv layer, shortcut and residual layer (``layer/<module name>``, taken
  with forward hooks; in ``pretrained_resnet_layers.npz`` / ``pretrained_resnet_b_layers.npz``, files of their own to stay under the size limit of a
  committed file), every decoder output (``dec/<i>``), the head output and the oracle's single-instance peaks on it;
  ``pretrained_resnet_b_state.npz``: B's state dict (A's is the run directory's checkpoint, stored as fp16 tensors: every value is drawn fp16-exact);
* ``tests/golden/ckpt_dirs/tiny_pretrained_resnet_single_instance``: ``best.ckpt`` + ``training_config.yaml`` + ``hf_config/config.json`` of A.

HuggingFace initialises BatchNorm to (weight 1, bias 0, mean 0, var 1), nearly the identity: every BatchNorm weight, bias, running_mean and running_var is
re-drawn (running_var uniform in 0.5 .. 2, means and biases O(0.3)), so that a missing or mis-ordered fold changes the golden.  The reference runs in ``eval()``.

    python tools/gen_pretrained_resnet_golden.py
"""
import os
import sys
import tempfile
import types

import numpy as np
import torch
import yaml

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_pretrained_golden as G  # noqa: E402  (frames(), the configs' layout and run() with its peak margins are that tool's)

GOLD = os.path.join(ROOT, "tests", "golden")
RUN_DIR = os.path.join(GOLD, "ckpt_dirs", "tiny_pretrained_resnet_single_instance")

CONFIGS = {
    # reduced widths 8 .. 32, a first layer with a projection shortcut at stride 1 (16 -> 32), identity shortcuts (the second layers)
    "A": {"layer_type": "bottleneck", "embedding_size": 16, "hidden_sizes": [32, 64, 96, 128], "depths": [2, 1, 2, 1], "output_stride": 2, "normalize": True,
          "filters_rate": 1.5, "seed": 303},
    # widths that are no multiples of 16; stage 0's first layer (24 -> 24, stride 1) has NO shortcut module
    "B": {"layer_type": "basic", "embedding_size": 24, "hidden_sizes": [24, 40, 48, 64], "depths": [2, 1, 1, 1], "output_stride": 4, "normalize": False,
          "filters_rate": 1.0, "seed": 404},
}
G.CONFIGS = CONFIGS  # backbone_config / head_config / run() read the table by name


def build(name, hf_dir, seed):
    import transformers  # noqa: F401  (before the harness: see tools/gen_pretrained_golden.py)
    from transformers import ResNetConfig

    c = CONFIGS[name]
    os.makedirs(hf_dir, exist_ok=True)
    ResNetConfig(num_channels=3, embedding_size=c["embedding_size"], hidden_sizes=c["hidden_sizes"], depths=c["depths"], layer_type=c["layer_type"], hidden_act="relu",
                 downsample_in_first_stage=False, downsample_in_bottleneck=False).save_pretrained(hf_dir)
    from oracle import ref_harness as rh

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
    bb = G.backbone_config(name, hf_dir)
    m = Model("pretrained", rh.attrdict(bb), rh.attrdict(G.head_config(name)), "single_instance").eval()
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for n, p in m.named_parameters():
            if ".normalization." in n:
                p.copy_((1.0 if n.endswith(".weight") else 0.0) + 0.3 * torch.randn(p.shape, generator=g))
            elif p.dim() > 1:
                torch.nn.init.kaiming_uniform_(p, a=1.0, generator=g)
            else:
                p.copy_(0.2 * (torch.rand(p.shape, generator=g) * 2 - 1))
        for n, b in m.named_buffers():
            if n.endswith(".running_mean"):
                b.copy_(0.3 * torch.randn(b.shape, generator=g))
            elif n.endswith(".running_var"):
                b.copy_(0.5 + 1.5 * torch.rand(b.shape, generator=g))
        # every value is rounded to one fp16 holds exactly: the run directory's checkpoint then stores fp16 tensors without loss (half the bytes: it has to stay under
        # the size limit of a committed file) and the reference computes the golden, in fp32, on exactly the values a loader reads back
        for t in list(m.parameters()) + [b for b in m.buffers() if b.is_floating_point()]:
            t.copy_(t.half().float())
    return m.eval(), bb


def run(name, m, img):
    """G.run's maps + the output of every ResNetConvLayer / ResNetShortCut / residual layer of the encoder, by module name."""
    layers, hooks = {}, []
    for n, mod in m.backbone.enc.named_modules():
        if type(mod).__name__ in ("ResNetConvLayer", "ResNetShortCut", "ResNetBasicLayer", "ResNetBottleNeckLayer"):
            def keep(_m, _i, o, n=n):  # (returns None: a hook's return value would replace the module's output)
                layers.setdefault("layer/backbone.enc." + n, o.detach().numpy().copy())

            hooks.append(mod.register_forward_hook(keep))
    try:
        out = G.run(name, m, img)
    finally:
        for h in hooks:
            h.remove()
    assert not m.backbone.enc.training and len(layers) > 8
    if CONFIGS[name]["layer_type"] == "bottleneck":  # a bottleneck's last conv before the add: covered by the layer's own output, and the largest share of the file
        layers = {k: v for k, v in layers.items() if not k.endswith(".layer.2")}
    return out, layers


def training_config(name):
    cfg = G.training_config(name)
    cfg["trainer_config"]["run_name"] = os.path.basename(RUN_DIR)
    return cfg


def main():
    os.makedirs(RUN_DIR, exist_ok=True)
    written = []
    with tempfile.TemporaryDirectory() as tmp:
        for name in CONFIGS:
            hf_dir = os.path.join(RUN_DIR, "hf_config") if name == "A" else os.path.join(tmp, "hf_" + name)
            for attempt in range(20):  # the first weight seed whose peaks are clear of their runners-up (the margin G.run asserts)
                m, _bb = build(name, hf_dir, CONFIGS[name]["seed"] + 1000 * attempt)
                try:
                    gold, layers = run(name, m, G.frames(CONFIGS[name]["seed"]))
                    break
                except AssertionError as e:
                    print(f"{name}: weight seed +{1000 * attempt} rejected: {e}")
            else:
                raise RuntimeError("no seed gives clear peaks")
            path = os.path.join(GOLD, "pretrained_resnet.npz" if name == "A" else "pretrained_resnet_b.npz")
            np.savez_compressed(path, **gold)
            written.append(path)
            path = path.replace(".npz", "_layers.npz")  # (a file of its own: together the maps pass the size limit)
            np.savez_compressed(path, **layers)
            written.append(path)
            if name == "A":
                half = lambda v: v.detach().half() if v.is_floating_point() else v.detach().clone()
                torch.save({"state_dict": {"model." + k: half(v) for k, v in m.state_dict().items()}}, os.path.join(RUN_DIR, "best.ckpt"))
                with open(os.path.join(RUN_DIR, "training_config.yaml"), "w") as f:
                    yaml.safe_dump(training_config(name), f, sort_keys=False)
                written.append(os.path.join(RUN_DIR, "best.ckpt"))
            else:
                path = os.path.join(GOLD, "pretrained_resnet_b_state.npz")
                np.savez_compressed(path, **{k: v.detach().numpy() for k, v in m.state_dict().items()})
                written.append(path)
    for p in written:
        assert os.path.getsize(p) < (1 << 20), p
        print(f"wrote {p} ({os.path.getsize(p) / 1024:.0f} KiB)")


if __name__ == "__main__":
    main()
