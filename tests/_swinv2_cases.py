"""What tools/gen_pretrained_swinv2_golden.py and the Swinv2 tests share, in pure NumPy: the fixture configurations, the seeded weights (head dimension 32 forces 32 / 64 /
128 / 256 channels, so a state dict is several MB: it is never committed, both sides draw it here) and the float64 statement of the cosine window attention that
tests/test_gpu_window_attn_v2.py holds the kernel to.

Every tensor is drawn from ``np.random.default_rng([seed, crc32(name)])``: its values depend on its name and shape alone, not on the order the caller lists them in.
"""
import math
import zlib

import numpy as np

PARTS = ["a", "b", "c"]
LOG100 = math.log(100.0)

# Fixture A: window 4 (16 tokens, T = 1); image_size 64 -> resolutions 16 / 8 / 4 / 2: stage 3 runs unshifted at window 4 and stage 4 shrinks to window 2.  Frames of
#   96 x 160 (not the config's size): maps 24x40 / 12x20 / 6x10 / 3x5, so stages 3 and 4 pad their windows.
# Fixture B: window 7 (49 tokens, T = 2 with dead key columns), image_size 224 -> resolutions 56 / 28 / 14 / 7: stage 4 unshifted; pretrained_window_sizes 6 normalise
#   the coordinate table.  Frames of 96 x 128: maps 24x32 / 12x16 / 6x8 / 3x4, every stage pads.
# W8: window 8 (N = 64 exactly), image_size 256 -> 64 / 32 / 16 / 8 (the published window8-256 geometry: stage 4 unshifted), no golden: held to tests/swinv2_ref.py.
FIXTURES = {
    "A": {"embed_dim": 32, "depths": [2, 2, 2, 2], "num_heads": [1, 2, 4, 8], "window_size": 4, "image_size": 64, "pretrained_window_sizes": [0, 0, 0, 0], "mlp_ratio": 2.0,
          "frame": (96, 160), "output_stride": 4, "normalize": True, "seed": 505},
    "B": {"embed_dim": 32, "depths": [2, 2, 2, 1], "num_heads": [1, 2, 4, 8], "window_size": 7, "image_size": 224, "pretrained_window_sizes": [6, 6, 6, 6], "mlp_ratio": 1.0,
          "frame": (96, 128), "output_stride": 8, "normalize": False, "seed": 606},
    "W8": {"embed_dim": 32, "depths": [2, 2, 1, 1], "num_heads": [1, 2, 4, 8], "window_size": 8, "image_size": 256, "pretrained_window_sizes": [0, 0, 0, 0], "mlp_ratio": 1.0,
           "frame": (64, 128), "output_stride": 8, "normalize": True, "seed": 707},
}
BATCH = 2


def hf_json(c, **over):
    """The fixture's ``config.json`` (settings only)."""
    return {"model_type": "swinv2", "image_size": c["image_size"], "patch_size": 4, "num_channels": 3, "embed_dim": c["embed_dim"], "depths": c["depths"], "num_heads": c["num_heads"],
            "window_size": c["window_size"], "pretrained_window_sizes": c["pretrained_window_sizes"], "mlp_ratio": c["mlp_ratio"], "qkv_bias": True, "hidden_act": "gelu",
            "use_absolute_embeddings": False, "layer_norm_eps": 1e-5, "drop_path_rate": 0.1, "hidden_dropout_prob": 0.0, "attention_probs_dropout_prob": 0.0, **over}


def backbone_config(name, model_name, allow=True):
    c = FIXTURES[name]
    bb = {"source": "hf", "model_name": model_name, "in_channels": 3, "output_stride": c["output_stride"], "max_stride": 32, "weights": False, "mode": "decoder",
          "out_indices": None, "freeze": False, "revision": None, "normalize": c["normalize"], "image_mean": None, "image_std": None, "filters_rate": 1.0,
          "convs_per_block": 1, "kernel_size": 3, "up_interpolate": True}
    if allow:
        bb["allow_swinv2"] = True
    return bb


def head_config(name):
    return {"confmaps": {"part_names": PARTS, "sigma": 2.5, "output_stride": FIXTURES[name]["output_stride"], "loss_weight": 1.0}}


def frames(name):
    """uint8 (BATCH, 3, H, W): blobs on noise; frame 1 at about 0.2 of frame 0's intensity (a reduction that wrongly spans the batch then changes the answer)."""
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


def draw_tensor(name, shape, seed):
    """One parameter, float32, from its name, shape and the seed."""
    g = np.random.default_rng([int(seed), zlib.crc32(name.encode())])
    shape = tuple(int(d) for d in shape)
    if name.endswith(".logit_scale"):
        # log 5 .. log 30; in every odd block one head sits ABOVE the clamp (log 150 -> scale 100, not 150): a missing clamp changes the golden
        v = g.uniform(math.log(5.0), math.log(30.0), size=shape)
        block = int(name.split(".blocks.")[1].split(".")[0])
        if block % 2 == 1:
            v.reshape(-1)[block % v.size] = math.log(150.0)
        return v.astype(np.float32)
    if ".continuous_position_bias_mlp." in name:
        if name.endswith(".0.weight"):
            return g.standard_normal(shape).astype(np.float32)
        if name.endswith(".0.bias"):
            return (0.5 * g.standard_normal(shape)).astype(np.float32)
        return (0.15 * g.standard_normal(shape)).astype(np.float32)  # .2.weight: the table's pre-sigmoid values spread over about +-2.5
    if "norm" in name and len(shape) == 1:  # embeddings.norm, layernorm_before / layernorm_after, downsample.norm
        return ((1.0 if name.endswith(".weight") else 0.0) + (0.3 if name.endswith(".weight") else 0.2) * g.standard_normal(shape)).astype(np.float32)
    if len(shape) > 1:
        fan_out, fan_in = shape[0] * int(np.prod(shape[2:], dtype=np.int64)), shape[1] * int(np.prod(shape[2:], dtype=np.int64))
        bound = math.sqrt(6.0 / (fan_in + fan_out)) * (2.0 if (".query." in name or ".key." in name or ".value." in name or ".dense." in name) else 1.0)
        return g.uniform(-bound, bound, size=shape).astype(np.float32)
    return (0.2 * g.uniform(-1.0, 1.0, size=shape)).astype(np.float32)


def draw_state(shapes, seed, keep=()):
    """``{name: float32 array}`` over ``shapes`` ({name: shape}); names in ``keep`` (the image statistics) are left to the caller."""
    return {k: draw_tensor(k, s, seed) for k, s in shapes.items() if k not in keep}


# ---- the cosine window attention, float64

def window_attn_v2_f64(qkv, qkv_bias, scale, table, heads, w, shift):
    """float64 statement of PH_OP_WINDOW_ATTN_V2 on an NHWC map.  ``qkv`` (B, H, W, 3C) = query | key | value, ``qkv_bias`` (3C) = the q, k, v of a padded token, ``scale``
    (heads), ``table`` (heads, (2w - 1)^2) indexed by (dy + w - 1)(2w - 1) + (dx + w - 1) with (dy, dx) = query - key position.  Pad to window multiples with padded
    tokens, roll by -shift on both axes, cut into windows; per head softmax(scale normalise(q) . normalise(k) + bias [- 200 between the bands of the last window row /
    column]) v; reverse, roll back, crop.  -> (B, H, W, C)."""
    qkv = np.asarray(qkv, dtype=np.float64)
    B, H, W, C3 = qkv.shape
    C = C3 // 3
    pH, pW = -(-H // w) * w, -(-W // w) * w
    x = np.broadcast_to(np.asarray(qkv_bias, dtype=np.float64), (B, pH, pW, C3)).copy()
    x[:, :H, :W] = qkv
    band = np.zeros((pH, pW), dtype=np.int64)
    if shift > 0:
        x = np.roll(x, (-shift, -shift), axis=(1, 2))
        hr = (np.arange(pH) >= pH - w).astype(np.int64) + (np.arange(pH) >= pH - shift)
        wr = (np.arange(pW) >= pW - w).astype(np.int64) + (np.arange(pW) >= pW - shift)
        band = hr[:, None] * 3 + wr[None, :]
    nh, nw, N = pH // w, pW // w, w * w
    win = x.reshape(B, nh, w, nw, w, C3).transpose(0, 1, 3, 2, 4, 5).reshape(B, nh * nw, N, C3)
    bw = band.reshape(nh, w, nw, w).transpose(0, 2, 1, 3).reshape(nh * nw, N)
    mask = np.where(bw[:, :, None] != bw[:, None, :], -200.0, 0.0)  # (windows, query, key)
    ty, tx = np.divmod(np.arange(N), w)
    idx = (ty[:, None] - ty[None, :] + w - 1) * (2 * w - 1) + (tx[:, None] - tx[None, :] + w - 1)
    out = np.empty((B, nh * nw, N, C))
    table = np.asarray(table, dtype=np.float64)
    for a in range(heads):
        q, k, v = (win[..., i * C + 32 * a: i * C + 32 * a + 32] for i in range(3))
        qn = q / np.maximum(np.sqrt((q * q).sum(-1, keepdims=True)), 1e-12)
        kn = k / np.maximum(np.sqrt((k * k).sum(-1, keepdims=True)), 1e-12)
        s = np.einsum("bwic,bwjc->bwij", qn, kn) * float(scale[a]) + table[a][idx][None, None] + mask[None]
        s = s - s.max(-1, keepdims=True)
        p = np.exp(s)
        p /= p.sum(-1, keepdims=True)
        out[..., 32 * a: 32 * a + 32] = np.einsum("bwij,bwjc->bwic", p, v)
    y = out.reshape(B, nh, nw, w, w, C).transpose(0, 1, 3, 2, 4, 5).reshape(B, pH, pW, C)
    if shift > 0:
        y = np.roll(y, (shift, shift), axis=(1, 2))
    return y[:, :H, :W]
