"""Generate the goldens of the Swinv2 fixtures with windows above 8 (C: window 16 of the 12to16 form, D: window 12; tests/_swinv2_wide_cases.py) from the reference's own
code, where the reference tree and ``transformers`` are available (CPU only, no network), on the pattern of tools/gen_pretrained_swinv2_golden.py and with the same
contents and labels:

* ``tests/golden/pretrained_swinv2_c.npz`` / ``pretrained_swinv2_d.npz``: the weight seed, the five encoder feature maps (``feat/<i>``), every decoder output
  (``dec/<i>``), the head output and the oracle's single-instance peaks on it;
* ``tests/golden/pretrained_swinv2_<c|d>_layers<k>.npz``: per block the attention branch back on the map, ``x1 = x + LayerNorm(.)`` and the block output, and every
  patch-merging output, for FRAME 1 ONLY, split greedily into files below the size limit.

The weights are NOT stored (tests/_swinv2_cases.draw_state draws them from the seed in the golden).  Fixture E (window 24) has no golden: the tests hold it to
tests/swinv2_ref.py.  The files of fixtures A and B are not touched.

    python tools/gen_pretrained_swinv2_wide_golden.py
"""
import glob
import json
import os
import sys
import tempfile
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_pretrained_golden as G  # noqa: E402  (run() with its peak margins is that tool's)
from tests import _swinv2_cases as SC  # noqa: E402
from tests import _swinv2_wide_cases as WC  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
LIMIT = 900 * 1024  # bytes of one committed file (under the 1 MiB limit with room)
KEEP = ("backbone.image_mean", "backbone.image_std")
G.CONFIGS = WC.FIXTURES  # run() reads output_stride by name


def build(name, hf_dir, seed):
    import transformers  # noqa: F401  (before the harness: see tools/gen_pretrained_golden.py)

    os.makedirs(hf_dir, exist_ok=True)
    with open(os.path.join(hf_dir, "config.json"), "w") as f:
        json.dump(WC.arch_of(name), f)
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
    m = Model("pretrained", rh.attrdict(WC.backbone_config(name, hf_dir, allow=False, wide=False)), rh.attrdict(WC.head_config(name)), "single_instance").eval()
    sd = m.state_dict()
    drawn = SC.draw_state({k: tuple(v.shape) for k, v in sd.items()}, seed, keep=KEEP)
    m.load_state_dict({**{k: sd[k] for k in KEEP}, **{k: torch.from_numpy(v) for k, v in drawn.items()}}, strict=True)
    return m.eval()


def run(name, m, img):
    """G.run's maps + the hooked block tensors of frame 1, by the program's label."""
    H, W = img.shape[-2:]
    layers, hooks = {}, []

    def nchw1(t, si):  # (B, h w, C) of stage si's map -> (1, C, h, w) of frame 1
        h, w = H // 4 // 2 ** si, W // 4 // 2 ** si
        assert t.shape[1] == h * w, (t.shape, h, w)
        return t.detach()[1:2].reshape(1, h, w, -1).permute(0, 3, 1, 2).contiguous().numpy().copy()

    def keep(label, si, pick):  # (a hook that returns None: a returned value would replace the module's input / output)
        def hook(_m, *io):
            layers.setdefault(label, nchw1(pick(io), si))

        return hook

    windows = []
    for n, mod in m.backbone.enc.named_modules():
        kind = type(mod).__name__
        label = "layer/backbone.enc." + n
        if kind == "Swinv2Layer":
            si = int(n.split("layers.")[1].split(".")[0])
            windows.append((int(mod.window_size), int(mod.shift_size)))
            hooks.append(mod.layernorm_before.register_forward_pre_hook(keep(label + ".attention", si, lambda io: io[0][0])))
            hooks.append(mod.intermediate.register_forward_pre_hook(keep(label + ".layernorm_before", si, lambda io: io[0][0])))
            hooks.append(mod.register_forward_hook(keep(label, si, lambda io: io[1][0])))
        elif kind == "Swinv2PatchMerging":
            si = int(n.split("layers.")[1].split(".")[0])
            hooks.append(mod.register_forward_hook(keep(label, si + 1, lambda io: io[1])))
    assert windows == WC.WINDOWS[name], (name, windows)  # the geometry the fixture was chosen for, as the reference's own layers hold it
    try:
        out = G.run(name, m, img)
    finally:
        for h in hooks:
            h.remove()
    assert not m.backbone.enc.training and len(layers) == 3 * sum(WC.FIXTURES[name]["depths"]) + 3
    return out, layers


def main():
    written = []
    for name in ("C", "D"):
        for old in glob.glob(os.path.join(GOLD, f"pretrained_swinv2_{name.lower()}*.npz")):
            os.remove(old)
    with tempfile.TemporaryDirectory() as tmp:
        for name in ("C", "D"):
            c = WC.FIXTURES[name]
            for attempt in range(20):  # the first weight seed whose peaks are clear of their runners-up (the margin G.run asserts)
                seed = c["seed"] + 1000 * attempt
                m = build(name, os.path.join(tmp, "hf_" + name), seed)
                try:
                    gold, layers = run(name, m, WC.frames(name))
                    break
                except AssertionError as e:
                    print(f"{name}: weight seed {seed} rejected: {e}")
            else:
                raise RuntimeError("no seed gives clear peaks")
            gold.pop("frames")  # (tests/_swinv2_wide_cases.frames draws them)
            gold["seed"] = np.int64(seed)
            stem = os.path.join(GOLD, f"pretrained_swinv2_{name.lower()}")
            np.savez_compressed(stem + ".npz", **gold)
            written.append(stem + ".npz")
            part, size, k = {}, 0, 0
            for key in sorted(layers):  # greedy split: float32 noise barely compresses, so the raw size is the estimate
                if part and size + layers[key].nbytes > LIMIT:
                    np.savez_compressed(f"{stem}_layers{k}.npz", **part)
                    written.append(f"{stem}_layers{k}.npz")
                    part, size, k = {}, 0, k + 1
                part[key] = layers[key]
                size += layers[key].nbytes
            np.savez_compressed(f"{stem}_layers{k}.npz", **part)
            written.append(f"{stem}_layers{k}.npz")
    for p in written:
        assert os.path.getsize(p) < LIMIT, p
        print(f"wrote {p} ({os.path.getsize(p) / 1024:.0f} KiB)")


if __name__ == "__main__":
    main()
