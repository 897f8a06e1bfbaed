"""What tools/gen_pretrained_swinv2_wide_golden.py and the tests of Swinv2 windows above 8 share, on top of tests/_swinv2_cases.py (whose weights, config.json form and
float64 statement of the attention they keep): the fixture configurations C, D and E, their frames, the operands of the kernel cases and the reference-order fp32
evaluation the kernel's bound is measured against.

``hf_order_fp32`` and ``operands`` restate those of tests/test_gpu_window_attn_v2.py (the bound is the same one: FOUR times the error of the reference's own fp32 order
against float64) so that the CPU tests can import them without a GPU module."""
import glob
import json
import os

import numpy as np
import torch
import torch.nn.functional as F

from tests import _swinv2_cases as SC
from tests import swinv2_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
ENC = "backbone.enc"
HEAD = "SingleInstanceConfmapsHead"

# Fixture C: window 16 (256 tokens, 8 key tiles), image_size 128 -> resolutions 32 / 16 / 8 / 4, pretrained_window_sizes of the 12to16 form.  Frames of 96 x 160: maps
#   24x40 / 12x20 / 6x10 / 3x5; stage 1 runs window 16 unshifted then shift 8 with both axes padded (24 -> 32, 40 -> 48), stage 2 window 16 unshifted on 12x20 padded to
#   16x32, stage 3 window 8 and stage 4 window 4 on the one-wave kernel.
# Fixture D: window 12 (144 tokens = 4 tiles + 16), image_size 96 -> 24 / 12 / 6 / 3, no pretrained windows.  Frames of 96 x 128: stage 1 window 12 shift 6, stage 2
#   window 12 unshifted, then windows 6 and 3.
# Fixture E: window 24 (576 tokens, 18 tiles), image_size 192 -> 48 / 24 / 12 / 6.  Frames of 64 x 96: stage 1 window 24 shift 12 on a 16x24 map, then 24 unshifted, 12, 6.
#   No golden: held to tests/swinv2_ref.py, as W8 is.
FIXTURES = {
    "C": {"embed_dim": 32, "depths": [2, 2, 1, 1], "num_heads": [1, 2, 4, 8], "window_size": 16, "image_size": 128, "pretrained_window_sizes": [12, 12, 12, 6], "mlp_ratio": 1.0,
          "frame": (96, 160), "output_stride": 8, "normalize": True, "seed": 808},
    "D": {"embed_dim": 32, "depths": [2, 2, 1, 1], "num_heads": [1, 2, 4, 8], "window_size": 12, "image_size": 96, "pretrained_window_sizes": [0, 0, 0, 0], "mlp_ratio": 2.0,
          "frame": (96, 128), "output_stride": 8, "normalize": False, "seed": 909},
    "E": {"embed_dim": 32, "depths": [2, 1, 1, 1], "num_heads": [1, 2, 4, 8], "window_size": 24, "image_size": 192, "pretrained_window_sizes": [12, 12, 12, 6], "mlp_ratio": 1.0,
          "frame": (64, 96), "output_stride": 8, "normalize": True, "seed": 1010},
}
# per block of the program: (window, shift), from the geometry above
WINDOWS = {"C": [(16, 0), (16, 8), (16, 0), (16, 0), (8, 0), (4, 0)], "D": [(12, 0), (12, 6), (12, 0), (12, 0), (6, 0), (3, 0)], "E": [(24, 0), (24, 12), (24, 0), (12, 0), (6, 0)]}
BATCH = SC.BATCH


def arch_of(name, **over):
    return SC.hf_json(FIXTURES[name], **over)


def backbone_config(name, model_name, allow=True, wide=True):
    c = FIXTURES[name]
    bb = {"source": "hf", "model_name": model_name, "in_channels": 3, "output_stride": c["output_stride"], "max_stride": 32, "weights": False, "mode": "decoder",
          "out_indices": None, "freeze": False, "revision": None, "normalize": c["normalize"], "image_mean": None, "image_std": None, "filters_rate": 1.0,
          "convs_per_block": 1, "kernel_size": 3, "up_interpolate": True}
    if allow:
        bb["allow_swinv2"] = True
    if wide:
        bb["allow_swinv2_wide"] = True
    return bb


def head_config(name):
    return {"confmaps": {"part_names": SC.PARTS, "sigma": 2.5, "output_stride": FIXTURES[name]["output_stride"], "loss_weight": 1.0}}


def frames(name):
    """uint8 (BATCH, 3, H, W), drawn as tests/_swinv2_cases.frames draws them: blobs on noise, frame 1 at about 0.2 of frame 0's intensity."""
    c = FIXTURES[name]
    H, W = c["frame"]
    g = np.random.default_rng(c["seed"])
    fr = 40.0 + 25.0 * g.standard_normal((BATCH, 3, H, W))
    yy, xx = np.mgrid[0:H, 0:W]
    for b in range(BATCH):
        for _ in range(4):
            cx, cy, s = g.uniform(8, W - 8), g.uniform(8, H - 8), g.uniform(3.0, 6.0)
            fr[b] += g.uniform(80, 200, size=(3, 1, 1)) * np.exp(-((xx - cx) ** 2 + (yy - cy) ** 2) / (2 * s * s))
    fr[1] *= 0.2
    return np.clip(fr, 0, 255).astype(np.uint8)


def hf_dir(name, tmp_path, **over):
    """A directory with the fixture's ``config.json``, written here (settings only)."""
    d = tmp_path / ("hf_" + name + "_".join(sorted(over)))
    d.mkdir(exist_ok=True)
    with open(d / "config.json", "w") as f:
        json.dump(arch_of(name, **over), f)
    return str(d)


def new_model(name, tmp_path, **bb_over):
    from sleap_nn_amd.architectures.model import Model

    return Model("pretrained", dict(backbone_config(name, hf_dir(name, tmp_path)), **bb_over), head_config(name), "single_instance")


def state_of(model, seed):
    """The seeded state dict over the model's parameter shapes + its image statistics as they stand."""
    sd = {k: torch.from_numpy(v) for k, v in SC.draw_state(model.param_shapes, seed).items()}
    sd.update({k: v.clone() for k, v in model.buffers.items()})
    return sd


_CACHE, _STATES = {}, {}


def golden(name):
    """The reference's outputs of fixture C or D (main file + the layer files as one dict), loaded once."""
    if name not in _CACHE:
        g = {}
        stem = os.path.join(GOLD, f"pretrained_swinv2_{name.lower()}")
        for f in [stem + ".npz"] + sorted(glob.glob(stem + "_layers*.npz")):
            z = np.load(f)
            g.update({k: z[k] for k in z.files})
        g["frames"] = frames(name)
        _CACHE[name] = g
    return _CACHE[name]


def fixture_state(name, tmp_path):
    """The state dict of a fixture, drawn once: from the golden's seed for C and D, from the fixture's own for E."""
    if name not in _STATES:
        seed = int(golden(name)["seed"]) if name in ("C", "D") else FIXTURES[name]["seed"]
        _STATES[name] = state_of(new_model(name, tmp_path), seed)
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
    heads["single_instance"] = head_config(name)
    pre = {"ensure_rgb": True, "ensure_grayscale": False, "max_height": None, "max_width": None, "scale": 1.0, "crop_size": None}
    cfg = {"data_config": {"preprocessing": pre, "skeletons": [{"name": "s", "nodes": [{"name": n} for n in SC.PARTS], "edges": []}]},
           "model_config": {"backbone_config": {"unet": None, "convnext": None, "swint": None, "pretrained": backbone_config(name, "hf_config", allow=False, wide=False)},
                            "head_configs": heads},
           "trainer_config": {"run_name": os.path.basename(str(path))}, "name": "", "description": "", "sleap_nn_version": "0.0.1"}
    with open(os.path.join(path, "training_config.yaml"), "w") as f:
        yaml.safe_dump(cfg, f, sort_keys=False)
    return str(path)


# ---- the kernel alone: cases, operands, the reference-order fp32 evaluation

# (window, shift, B, H, W, heads, one head at the scale clamp, an all-zero token inside the map)
KERNEL_CASES = [
    (9, 0, 1, 9, 9, 1, False, False),      # 81 tokens: the last tile has 17 live keys, wave 3 has no query tile
    (9, 4, 2, 10, 19, 3, True, True),
    (12, 0, 1, 12, 12, 3, False, True),
    (12, 6, 2, 13, 25, 1, False, False),
    (16, 0, 2, 16, 16, 3, False, False),   # 8 full tiles
    (16, 8, 2, 16, 32, 2, True, False),    # one window covers H, rolled and masked anyway
    (16, 8, 1, 20, 36, 1, False, True),
    (24, 0, 1, 24, 24, 3, False, False),
    (24, 12, 1, 24, 48, 1, True, False),
    (24, 12, 1, 30, 25, 2, False, True),
    (8, 4, 2, 13, 9, 3, False, False),     # windows of 2..8: the same statement, the same bound, the new kernel
    (7, 3, 2, 9, 15, 3, False, False),
    (2, 1, 2, 5, 7, 3, False, False),      # N = 4: a single partial tile
    (15, 7, 1, 15, 15, 1, False, False),   # 225 tokens: the last tile holds ONE live key (the lane half 1 of that tile has none)
]


def case_id(c):
    return "w%d_s%d_b%d_%dx%d_h%d%s%s" % (c[:6] + ("_clamp" if c[6] else "", "_zero" if c[7] else ""))


def operands(case):
    w, shift, B, H, W, heads, clamp, zero = case
    g = np.random.default_rng([w, shift, H, W, heads])
    Cc = 32 * heads
    qkv = g.standard_normal((B, H, W, 3 * Cc)).astype(np.float32)
    qkv[..., :Cc] *= g.uniform(0.2, 3.0, size=(B, H, W, 1)).astype(np.float32)  # token norms differ: a missing normalisation shows
    if zero:
        qkv[B - 1, H // 2, W // 2, :] = 0.0  # q = k = v = 0: its normalised k is 0 / 1e-12 = 0
    bias = (0.5 * g.standard_normal(3 * Cc)).astype(np.float32)
    bias[Cc:2 * Cc] = 0.0  # key has no bias: a padded token's k is exactly 0
    scale = g.uniform(5.0, 30.0, size=heads).astype(np.float32)
    if clamp:
        scale[heads - 1] = 100.0
    table = (16.0 / (1.0 + np.exp(-2.0 * g.standard_normal((heads, (2 * w - 1) ** 2))))).astype(np.float32)
    return qkv, bias, scale, table


def hf_order_fp32(qkv, bias, scale, table, heads, w, shift):
    """The same operation in torch on the CPU, fp32, in the order of Swinv2Layer / Swinv2SelfAttention.forward (on a qkv map: a padded token's q, k, v are ``bias``);
    the mask is added twice, as the installed layer does."""
    x = torch.from_numpy(qkv)
    B, H, W, C3 = x.shape
    Cc = C3 // 3
    pH, pW = -(-H // w) * w, -(-W // w) * w
    full = torch.from_numpy(bias).expand(B, pH, pW, C3).clone()
    full[:, :H, :W] = x
    if shift > 0:
        full = torch.roll(full, shifts=(-shift, -shift), dims=(1, 2))
    win = R.partition(full, w).view(-1, w * w, C3)
    Bn, N = win.shape[0], w * w
    q, k, v = (win[..., i * Cc:(i + 1) * Cc].reshape(Bn, N, heads, 32).transpose(1, 2) for i in range(3))
    s = F.normalize(q, dim=-1) @ F.normalize(k, dim=-1).transpose(-2, -1)
    s = s * torch.from_numpy(scale).view(heads, 1, 1)
    s = s + torch.from_numpy(table)[:, R.position_index(w).view(-1)].view(heads, N, N).unsqueeze(0)
    mask = R.shift_mask(pH, pW, w, shift, torch.float32)
    if mask is not None:
        nm = mask.shape[0]
        s = s.view(Bn // nm, nm, heads, N, N) + mask.unsqueeze(1).unsqueeze(0)
        s = s + mask.unsqueeze(1).unsqueeze(0)
        s = s.view(-1, heads, N, N)
    ctx = (F.softmax(s, dim=-1) @ v).permute(0, 2, 1, 3).contiguous().view(Bn, N, Cc)
    y = R.reverse(ctx.view(-1, w, w, Cc), w, pH, pW)
    if shift > 0:
        y = torch.roll(y, shifts=(shift, shift), dims=(1, 2))
    return y[:, :H, :W].contiguous().numpy()


def forced_rescale_operands(w):
    """One unshifted w x w window, one head at scale 30, a flat bias table: the running maximum of two chosen queries is forced to move.
    Query A (token 5): every key is near-orthogonal to it but the LAST token, whose k is A's q direction -- the maximum jumps in the last key tile, by about the scale.
    Query B (token 40): key j's cosine with it rises with j (from -0.9 to 0.9) -- the maximum rises at every tile.  -> operands, (token A, token B)."""
    N = w * w
    g = np.random.default_rng([77, w])
    qkv = g.standard_normal((1, w, w, 96)).astype(np.float32)
    flat = qkv.reshape(N, 96)
    ta, tb = 5, 40
    qa = flat[ta, :32].astype(np.float64)
    qa /= np.linalg.norm(qa)
    qb = flat[tb, :32].astype(np.float64)
    qb -= qa * (qa @ qb)  # B's query direction, orthogonal to A's: the two constructions do not disturb each other
    qb /= np.linalg.norm(qb)
    flat[tb, :32] = (2.0 * qb).astype(np.float32)
    cos = np.linspace(-0.9, 0.9, N)
    for j in range(N):
        r = g.standard_normal(32)
        r -= qa * (qa @ r) + qb * (qb @ r)
        r /= np.linalg.norm(r)
        k = cos[j] * qb + np.sqrt(1.0 - cos[j] ** 2) * r  # cosine cos[j] with B's query, 0 with A's
        flat[j, 32:64] = (g.uniform(0.5, 2.0) * k).astype(np.float32)
    flat[N - 1, 32:64] = (1.5 * qa).astype(np.float32)  # the one key aligned with A's query: in the last tile
    bias = (0.5 * g.standard_normal(96)).astype(np.float32)
    bias[32:64] = 0.0
    scale = np.array([30.0], dtype=np.float32)
    table = np.full((1, (2 * w - 1) ** 2), 8.0, dtype=np.float32)
    return (qkv, bias, scale, table), (ta, tb)
