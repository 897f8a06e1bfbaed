"""Plain-torch restatement of HuggingFace's ``Swinv2Backbone`` and of Case A (``mode="decoder"``) of the reference ``PretrainedBackbone``
(sleap_nn/architectures/pretrained.py), in the role tests/resnet_ref.py has for the ResNet family.  UNDERIVED: the continuous-position-bias MLP, the clamp and exp of
``logit_scale`` and the three separate query / key / value Linears are evaluated as HuggingFace evaluates them, in its order, so a wrong derived form in the program shows.

It needs neither ``transformers`` nor the reference tree: tests/test_pretrained_swinv2_cpu.py compares it with the reference's own outputs
(tests/golden/pretrained_swinv2*.npz) and, where ``transformers`` is installed, with ``Swinv2Backbone`` directly.  State-dict keys are the reference's.  ``arch`` is the
``config.json`` dictionary (tests/_swinv2_cases.hf_json)."""
import math
from typing import Dict, List, Optional

import torch
import torch.nn.functional as F

from oracle import cpu_ref as O

ENC = "backbone.enc"


def windows_of(arch) -> List[tuple]:
    """Per stage (window, shift of the odd blocks): Swinv2Layer._compute_window_shift on the config's image_size (the height axis' values, as HuggingFace keeps them)."""
    img = arch["image_size"]
    ih = int(img[0] if isinstance(img, (list, tuple)) else img)
    out = []
    for i in range(len(arch["depths"])):
        res = ih // int(arch["patch_size"]) // 2 ** i
        w = min(res, int(arch["window_size"]))
        out.append((w, 0 if res <= w else int(arch["window_size"]) // 2))
    return out


def coords_table(window: int, pretrained_window: int, dtype=torch.float32) -> torch.Tensor:
    """Swinv2SelfAttention.create_coords_table_and_index: (1, 2w - 1, 2w - 1, 2)."""
    r = torch.arange(-(window - 1), window, dtype=torch.int64).float()
    t = torch.stack(torch.meshgrid([r, r], indexing="ij")).permute(1, 2, 0).contiguous().unsqueeze(0)
    if pretrained_window > 0:
        t[:, :, :, 0] /= pretrained_window - 1
        t[:, :, :, 1] /= pretrained_window - 1
    elif window > 1:
        t[:, :, :, 0] /= window - 1
        t[:, :, :, 1] /= window - 1
    t *= 8
    t = torch.sign(t) * torch.log2(torch.abs(t) + 1.0) / math.log2(8)
    return t.to(dtype)


def position_index(window: int) -> torch.Tensor:
    c = torch.stack(torch.meshgrid([torch.arange(window), torch.arange(window)], indexing="ij")).flatten(1)
    rel = (c[:, :, None] - c[:, None, :]).permute(1, 2, 0).contiguous()
    rel[:, :, 0] += window - 1
    rel[:, :, 1] += window - 1
    rel[:, :, 0] *= 2 * window - 1
    return rel.sum(-1)


def partition(x: torch.Tensor, w: int) -> torch.Tensor:
    B, H, W, C = x.shape
    return x.view(B, H // w, w, W // w, w, C).permute(0, 1, 3, 2, 4, 5).contiguous().view(-1, w, w, C)


def reverse(win: torch.Tensor, w: int, H: int, W: int) -> torch.Tensor:
    C = win.shape[-1]
    return win.view(-1, H // w, W // w, w, w, C).permute(0, 1, 3, 2, 4, 5).contiguous().view(-1, H, W, C)


def shift_mask(H: int, W: int, w: int, shift: int, dtype) -> Optional[torch.Tensor]:
    """Swinv2Layer.get_attn_mask: (windows, N, N) of 0 / -100, None for an unshifted layer."""
    if shift <= 0:
        return None
    hr = (torch.arange(H) >= H - w).long() + (torch.arange(H) >= H - shift).long()
    wr = (torch.arange(W) >= W - w).long() + (torch.arange(W) >= W - shift).long()
    img = (hr[None, :, None, None] * 3 + wr[None, None, :, None]).to(dtype)
    mw = partition(img, w).view(-1, w * w)
    m = mw.unsqueeze(1) - mw.unsqueeze(2)
    return m.masked_fill(m != 0, -100.0).masked_fill(m == 0, 0.0)


def self_attention(sd, a: str, hs: torch.Tensor, mask: Optional[torch.Tensor], heads: int, window: int, pretrained_window: int) -> torch.Tensor:
    """Swinv2SelfAttention.forward on windows ``hs`` (windows * B, N, C), in its order of operations -- the mask is added TWICE, as the installed transformers does."""
    Bn, N, C = hs.shape
    d = C // heads
    q = F.linear(hs, sd[a + ".query.weight"], sd[a + ".query.bias"]).view(Bn, N, heads, d).transpose(1, 2)
    k = F.linear(hs, sd[a + ".key.weight"]).view(Bn, N, heads, d).transpose(1, 2)
    v = F.linear(hs, sd[a + ".value.weight"], sd[a + ".value.bias"]).view(Bn, N, heads, d).transpose(1, 2)
    s = F.normalize(q, dim=-1) @ F.normalize(k, dim=-1).transpose(-2, -1)
    s = s * torch.clamp(sd[a + ".logit_scale"], max=math.log(1.0 / 0.01)).exp()
    m = a + ".continuous_position_bias_mlp"
    t = F.linear(F.relu(F.linear(coords_table(window, pretrained_window, hs.dtype), sd[m + ".0.weight"], sd[m + ".0.bias"])), sd[m + ".2.weight"]).view(-1, heads)
    bias = t[position_index(window).view(-1)].view(N, N, -1).permute(2, 0, 1).contiguous()
    s = s + (16 * torch.sigmoid(bias)).unsqueeze(0)
    if mask is not None:
        nm = mask.shape[0]
        s = s.view(Bn // nm, nm, heads, N, N) + mask.unsqueeze(1).unsqueeze(0)
        s = s + mask.unsqueeze(1).unsqueeze(0)
        s = s.view(-1, heads, N, N)
    p = F.softmax(s, dim=-1)
    return (p @ v).permute(0, 2, 1, 3).contiguous().view(Bn, N, C)


def block_forward(sd, n: str, x: torch.Tensor, heads: int, window: int, shift: int, pretrained_window: int, eps: float, collect: Optional[dict] = None) -> torch.Tensor:
    """Swinv2Layer.forward on an NHWC map ``x`` (B, H, W, C)."""
    B, H, W, C = x.shape
    pr, pb = (window - W % window) % window, (window - H % window) % window
    hs = F.pad(x, (0, 0, 0, pr, 0, pb))
    pH, pW = hs.shape[1], hs.shape[2]
    if shift > 0:
        hs = torch.roll(hs, shifts=(-shift, -shift), dims=(1, 2))
    win = partition(hs, window).view(-1, window * window, C)
    ctx = self_attention(sd, n + ".attention.self", win, shift_mask(pH, pW, window, shift, x.dtype), heads, window, pretrained_window)

    def to_map(t):
        t = reverse(t.view(-1, window, window, C), window, pH, pW)
        if shift > 0:
            t = torch.roll(t, shifts=(shift, shift), dims=(1, 2))
        return t[:, :H, :W, :].contiguous()

    att = to_map(F.linear(ctx, sd[n + ".attention.output.dense.weight"], sd[n + ".attention.output.dense.bias"]))
    x1 = x + F.layer_norm(att, (C,), sd[n + ".layernorm_before.weight"], sd[n + ".layernorm_before.bias"], eps)
    h = F.gelu(F.linear(x1, sd[n + ".intermediate.dense.weight"], sd[n + ".intermediate.dense.bias"]))
    o = F.linear(h, sd[n + ".output.dense.weight"], sd[n + ".output.dense.bias"])
    x2 = x1 + F.layer_norm(o, (C,), sd[n + ".layernorm_after.weight"], sd[n + ".layernorm_after.bias"], eps)
    if collect is not None:
        nchw = lambda t: t.permute(0, 3, 1, 2).contiguous()
        collect[n + ".attention.self"] = nchw(to_map(ctx))
        collect[n + ".attention"] = nchw(att)
        collect[n + ".layernorm_before"] = nchw(x1)
        collect[n + ".intermediate"] = nchw(h)
        collect[n + ".output"] = nchw(o)
        collect[n] = nchw(x2)
    return x2


def merge_forward(sd, n: str, x: torch.Tensor, collect: Optional[dict] = None) -> torch.Tensor:
    """Swinv2PatchMerging.forward on an NHWC map: gather (zeros past an odd edge) -> reduction (no bias) -> LayerNorm (eps 1e-5, the module default)."""
    B, H, W, C = x.shape
    x = F.pad(x, (0, 0, 0, W % 2, 0, H % 2))
    g = torch.cat([x[:, 0::2, 0::2, :], x[:, 1::2, 0::2, :], x[:, 0::2, 1::2, :], x[:, 1::2, 1::2, :]], -1)
    r = F.linear(g, sd[n + ".reduction.weight"])
    y = F.layer_norm(r, (2 * C,), sd[n + ".norm.weight"], sd[n + ".norm.bias"], 1e-5)
    if collect is not None:
        collect[n + ".reduction"] = r.permute(0, 3, 1, 2).contiguous()
        collect[n] = y.permute(0, 3, 1, 2).contiguous()
    return y


def encoder_forward(sd, arch: dict, x: torch.Tensor, collect: Optional[dict] = None, prefix: str = ENC) -> List[torch.Tensor]:
    """``Swinv2Backbone(out_features=all)(x).feature_maps``: [stem, stage1..4] in NCHW, the stage maps RAW and before the downsampling.  ``x``: (B, C, H, W), already normalised."""
    if prefix != ENC:
        sd = {ENC + k[len(prefix):]: v for k, v in sd.items() if k.startswith(prefix)}
    pe = f"{ENC}.embeddings.patch_embeddings.projection"
    p = int(arch["patch_size"])
    y = F.conv2d(x, sd[pe + ".weight"], sd[pe + ".bias"], stride=p)
    if collect is not None:
        collect[pe] = y
    y = y.permute(0, 2, 3, 1)
    C = y.shape[-1]
    y = F.layer_norm(y, (C,), sd[f"{ENC}.embeddings.norm.weight"], sd[f"{ENC}.embeddings.norm.bias"], 1e-5)
    feats = [y.permute(0, 3, 1, 2).contiguous()]
    eps = float(arch.get("layer_norm_eps", 1e-5))
    pws = arch.get("pretrained_window_sizes") or [0, 0, 0, 0]
    for si, ((w, shift), depth, heads) in enumerate(zip(windows_of(arch), arch["depths"], arch["num_heads"])):
        for j in range(depth):
            y = block_forward(sd, f"{ENC}.encoder.layers.{si}.blocks.{j}", y, heads, w, 0 if j % 2 == 0 else shift, int(pws[si]), eps, collect)
        feats.append(y.permute(0, 3, 1, 2).contiguous())
        if si + 1 < len(arch["depths"]):
            y = merge_forward(sd, f"{ENC}.encoder.layers.{si}.downsample", y, collect)
    return feats


def backbone_forward(sd, bb: dict, arch: dict, x: torch.Tensor, collect: Optional[dict] = None) -> dict:
    """``PretrainedBackbone.forward``, Case A, as tests/resnet_ref.py states it: the last map of every size, UNet-style decoder over them.  ``x`` in [0, 1]."""
    if bb.get("normalize", True):
        x = (x - sd["backbone.image_mean"]) / sd["backbone.image_std"]
    feats = encoder_forward(sd, arch, x, collect)
    by_size = {}
    for f in feats:  # the stem map shares its size with stage1 and gives way to it
        by_size[f.shape[-2]] = f
    maps = [by_size[h] for h in sorted(by_size, reverse=True)]
    bottleneck, skips = maps[-1], maps[:-1][::-1]
    stride = x.shape[-2] // bottleneck.shape[-2]
    up_blocks = int(math.log2(stride / int(bb.get("output_stride", 2))))
    cur, outs, strides = bottleneck, [], []
    for b in range(up_blocks):
        nxt = stride // 2
        name = f"backbone.dec.decoder_stack.{b}.blocks.pretrained_dec{b}_s{stride}_to_s{nxt}"
        cur = F.interpolate(cur, scale_factor=2, mode="bilinear", align_corners=False)
        if b < len(skips):
            cur = torch.cat((skips[b], cur), dim=1)
        i = 0
        while name + f"_refine_conv{i}.weight" in sd:
            cur = F.relu(F.conv2d(cur, sd[name + f"_refine_conv{i}.weight"], sd[name + f"_refine_conv{i}.bias"], padding=1))
            if collect is not None:
                collect[name + f"_refine_conv{i}"] = cur
            i += 1
        outs.append(cur)
        strides.append(nxt)
        stride = nxt
    return {"outputs": outs, "strides": strides, "middle_output": bottleneck, "feature_maps": feats}


def model_forward(sd, bb: dict, arch: dict, head_cfgs: dict, model_type: str, image: torch.Tensor, collect: Optional[dict] = None) -> Dict[str, torch.Tensor]:
    x = O.normalize_input(image)
    bo = backbone_forward(sd, bb, arch, x, collect)
    out = {}
    for i, (hname, key) in enumerate(O.HEAD_ORDER[model_type]):
        hc = head_cfgs[key]
        feat = bo["outputs"][bo["strides"].index(hc["output_stride"])]
        out[hname] = F.conv2d(feat, sd[f"head_layers.{i}.{hname}.0.weight"], sd[f"head_layers.{i}.{hname}.0.bias"])
    return out
