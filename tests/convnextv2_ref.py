"""Plain-torch restatement of HuggingFace's ``ConvNextV2Backbone`` and of Case A (``mode="decoder"``) of the reference
``PretrainedBackbone`` (sleap_nn/architectures/pretrained.py), in the role tests/swin_ref.py has for the Swin path.

It needs neither ``transformers`` nor the reference tree: tests/test_pretrained_cpu.py compares it with the reference's own
outputs (tests/golden/pretrained_convnextv2.npz) and, where ``transformers`` is installed, with ``ConvNextV2Backbone`` directly.
State-dict keys are the reference's (``backbone.enc...``, ``backbone.dec...``, ``backbone.image_mean`` / ``image_std``).
"""
import math
from typing import Dict, List, Optional

import torch
import torch.nn.functional as F

from oracle import cpu_ref as O

ENC = "backbone.enc"
EPS = 1e-6


def grn(x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor) -> torch.Tensor:
    """ConvNextV2GRN on a (B, H, W, C) tensor."""
    g = torch.linalg.vector_norm(x, ord=2, dim=(1, 2), keepdim=True)
    n = g / (g.mean(dim=-1, keepdim=True) + 1e-6)
    return weight * (x * n) + bias + x


def v2_block(sd, n: str, x: torch.Tensor, collect: Optional[dict] = None) -> torch.Tensor:
    """ConvNextV2Layer, ``x`` (B, C, H, W); drop path is the identity in eval."""
    c = x.shape[1]
    y = F.conv2d(x, sd[n + ".dwconv.weight"], sd[n + ".dwconv.bias"], padding=3, groups=c).permute(0, 2, 3, 1)
    y = F.layer_norm(y, (c,), sd[n + ".layernorm.weight"], sd[n + ".layernorm.bias"], EPS)
    y = F.gelu(F.linear(y, sd[n + ".pwconv1.weight"], sd[n + ".pwconv1.bias"]))
    y = grn(y, sd[n + ".grn.weight"], sd[n + ".grn.bias"])
    if collect is not None:
        collect[n + ".grn"] = y.permute(0, 3, 1, 2)
    y = F.linear(y, sd[n + ".pwconv2.weight"], sd[n + ".pwconv2.bias"]).permute(0, 3, 1, 2)
    return x + y


def ln_cf(x: torch.Tensor, w: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """Channels-first LayerNorm (ConvNextV2LayerNorm, data_format="channels_first")."""
    return F.layer_norm(x.permute(0, 2, 3, 1), (x.shape[1],), w, b, EPS).permute(0, 3, 1, 2)


def depths_of(sd) -> List[int]:
    d = [0, 0, 0, 0]
    for k in sd:
        if k.startswith(f"{ENC}.encoder.stages.") and k.endswith(".dwconv.weight"):
            p = k.split(".")
            d[int(p[4])] = max(d[int(p[4])], int(p[6]) + 1)
    return d


def encoder_forward(sd, x: torch.Tensor, collect: Optional[dict] = None, prefix: str = ENC) -> List[torch.Tensor]:
    """``ConvNextV2Backbone(out_indices=all)(x).feature_maps``: [stem, stage1..4], each through its own ``hidden_states_norms`` entry.
    ``x``: (B, 3, H, W), already normalised.  The norm is applied to the copy that leaves, not to the stream into the next stage."""
    if prefix != ENC:
        sd = {ENC + k[len(prefix):]: v for k, v in sd.items() if k.startswith(prefix)}
    pw = sd[f"{ENC}.embeddings.patch_embeddings.weight"]
    x = F.conv2d(x, pw, sd[f"{ENC}.embeddings.patch_embeddings.bias"], stride=pw.shape[-1])
    x = ln_cf(x, sd[f"{ENC}.embeddings.layernorm.weight"], sd[f"{ENC}.embeddings.layernorm.bias"])
    if collect is not None:
        collect[f"{ENC}.embeddings"] = x
    hn = f"{ENC}.hidden_states_norms"
    feats = [ln_cf(x, sd[f"{hn}.stem.weight"], sd[f"{hn}.stem.bias"])]
    for si, depth in enumerate(depths_of(sd)):
        st = f"{ENC}.encoder.stages.{si}"
        if si > 0:
            x = ln_cf(x, sd[f"{st}.downsampling_layer.0.weight"], sd[f"{st}.downsampling_layer.0.bias"])
            x = F.conv2d(x, sd[f"{st}.downsampling_layer.1.weight"], sd[f"{st}.downsampling_layer.1.bias"], stride=2)
        for j in range(depth):
            x = v2_block(sd, f"{st}.layers.{j}", x, collect)
            if collect is not None:
                collect[f"{st}.layers.{j}"] = x
        f = ln_cf(x, sd[f"{hn}.stage{si + 1}.weight"], sd[f"{hn}.stage{si + 1}.bias"])
        if collect is not None:
            collect[f"{hn}.stage{si + 1}"] = f
        feats.append(f)
    return feats


def backbone_forward(sd, bb: dict, x: torch.Tensor, collect: Optional[dict] = None) -> dict:
    """``PretrainedBackbone.forward`` (pretrained.py:471-502), Case A.  ``x``: (B, 3, H, W) in [0, 1]."""
    if bb.get("normalize", True):
        x = (x - sd["backbone.image_mean"]) / sd["backbone.image_std"]
    feats = encoder_forward(sd, x, collect)
    by_size = {}
    for f in feats:  # _select_pyramid: the last map of every size, finest first (the stem map gives way to stage1)
        by_size[f.shape[-2]] = f
    maps = [by_size[h] for h in sorted(by_size, reverse=True)]
    bottleneck, skips = maps[-1], maps[:-1][::-1]
    stride = x.shape[-2] // bottleneck.shape[-2]
    up_blocks = int(math.log2(stride / int(bb.get("output_stride", 2))))
    cur, outs, strides = bottleneck, [], []
    for b in range(up_blocks):
        nxt = stride // 2
        name = f"backbone.dec.decoder_stack.{b}.blocks.pretrained_dec{b}_s{stride}_to_s{nxt}"
        if bb.get("up_interpolate", True):
            cur = F.interpolate(cur, scale_factor=2, mode="bilinear", align_corners=False)
        else:
            cur = F.relu(F.conv_transpose2d(cur, sd[name + "_trans_conv.weight"], sd[name + "_trans_conv.bias"], stride=2, padding=1, output_padding=1))
            if collect is not None:
                collect[name + "_trans_conv"] = cur
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


def model_forward(sd, bb: dict, head_cfgs: dict, model_type: str, image: torch.Tensor, collect: Optional[dict] = None) -> Dict[str, torch.Tensor]:
    """``Model.forward`` with this backbone (confidence-map / PAF / offset heads: plain 1x1 convolutions).  A 1-channel frame is replicated."""
    x = O.normalize_input(image)
    if x.shape[-3] == 1:
        x = x.repeat(1, 3, 1, 1)
    bo = backbone_forward(sd, bb, x, collect)
    out = {}
    for i, (hname, key) in enumerate(O.HEAD_ORDER[model_type]):
        hc = head_cfgs[key]
        feat = bo["outputs"][bo["strides"].index(hc["output_stride"])]
        out[hname] = F.conv2d(feat, sd[f"head_layers.{i}.{hname}.0.weight"], sd[f"head_layers.{i}.{hname}.0.bias"])
    return out
