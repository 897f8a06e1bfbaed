"""Plain-torch restatement of HuggingFace's ``ResNetBackbone`` and of Case A (``mode="decoder"``) of the reference ``PretrainedBackbone``
(sleap_nn/architectures/pretrained.py), in the role tests/convnextv2_ref.py has for the ConvNeXtV2 family.  UNFOLDED: every conv is followed by real
BatchNorm arithmetic in eval mode (``F.batch_norm`` on the running statistics), so a wrong fold in the program shows against it.

It needs neither ``transformers`` nor the reference tree: tests/test_pretrained_resnet_cpu.py compares it with the reference's own outputs
(tests/golden/pretrained_resnet*.npz) and, where ``transformers`` is installed, with ``ResNetBackbone`` directly.  State-dict keys are the reference's.
"""
import math
from typing import Dict, List, Optional

import torch
import torch.nn.functional as F

from oracle import cpu_ref as O

ENC = "backbone.enc"
BN_EPS = 1e-5


def conv_bn(sd, n: str, x: torch.Tensor, stride: int = 1, relu: bool = True) -> torch.Tensor:
    """ResNetConvLayer / ResNetShortCut: Conv2d(bias=False, padding k // 2) -> BatchNorm2d (eval) (-> ReLU)."""
    w = sd[n + ".convolution.weight"]
    y = F.conv2d(x, w, None, stride=stride, padding=w.shape[-1] // 2)
    b = n + ".normalization"
    y = F.batch_norm(y, sd[b + ".running_mean"], sd[b + ".running_var"], sd[b + ".weight"], sd[b + ".bias"], False, 0.0, BN_EPS)
    return F.relu(y) if relu else y


def layer_forward(sd, n: str, x: torch.Tensor, stride: int, collect: Optional[dict] = None) -> torch.Tensor:
    """ResNetBasicLayer (two convs) or ResNetBottleNeckLayer (three), told apart by the keys; the stride sits on the first 3x3 conv."""
    res = conv_bn(sd, n + ".shortcut", x, stride, relu=False) if n + ".shortcut.convolution.weight" in sd else x
    if collect is not None and res is not x:
        collect[n + ".shortcut"] = res
    k = 0
    convs = []
    while f"{n}.layer.{k}.convolution.weight" in sd:
        convs.append(f"{n}.layer.{k}")
        k += 1
    strided = next(i for i, c in enumerate(convs) if sd[c + ".convolution.weight"].shape[-1] == 3)  # basic: layer.0, bottleneck: layer.1
    y = x
    for i, c in enumerate(convs):
        y = conv_bn(sd, c, y, stride if i == strided else 1, relu=i + 1 < len(convs))
        if collect is not None:
            collect[c] = y  # (the last conv's entry is the value BEFORE the add)
    y = F.relu(y + res)
    if collect is not None:
        collect[n] = y
    return y


def depths_of(sd) -> List[int]:
    d = [0, 0, 0, 0]
    for k in sd:
        if k.startswith(f"{ENC}.encoder.stages.") and k.endswith(".layer.0.convolution.weight"):
            p = k.split(".")
            d[int(p[4])] = max(d[int(p[4])], int(p[6]) + 1)
    return d


def encoder_forward(sd, x: torch.Tensor, collect: Optional[dict] = None, prefix: str = ENC) -> List[torch.Tensor]:
    """``ResNetBackbone(out_indices=all)(x).feature_maps``: [stem, stage1..4], RAW (no output norms).  ``x``: (B, C, H, W), already normalised."""
    if prefix != ENC:
        sd = {ENC + k[len(prefix):]: v for k, v in sd.items() if k.startswith(prefix)}
    x = conv_bn(sd, f"{ENC}.embedder.embedder", x, 2)
    if collect is not None:
        collect[f"{ENC}.embedder.embedder"] = x
    x = F.max_pool2d(x, 3, 2, 1)
    feats = [x]
    for si, depth in enumerate(depths_of(sd)):
        for j in range(depth):
            x = layer_forward(sd, f"{ENC}.encoder.stages.{si}.layers.{j}", x, 2 if (si > 0 and j == 0) else 1, collect)
        feats.append(x)
    return feats


def backbone_forward(sd, bb: dict, x: torch.Tensor, collect: Optional[dict] = None) -> dict:
    """``PretrainedBackbone.forward``, Case A, as tests/convnextv2_ref.py states it: the last map of every size, UNet-style decoder over them.  ``x`` in [0, 1]."""
    if bb.get("normalize", True):
        x = (x - sd["backbone.image_mean"]) / sd["backbone.image_std"]
    feats = encoder_forward(sd, x, collect)
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


def model_forward(sd, bb: dict, head_cfgs: dict, model_type: str, image: torch.Tensor, collect: Optional[dict] = None) -> Dict[str, torch.Tensor]:
    x = O.normalize_input(image)
    bo = backbone_forward(sd, bb, x, collect)
    out = {}
    for i, (hname, key) in enumerate(O.HEAD_ORDER[model_type]):
        hc = head_cfgs[key]
        feat = bo["outputs"][bo["strides"].index(hc["output_stride"])]
        out[hname] = F.conv2d(feat, sd[f"head_layers.{i}.{hname}.0.weight"], sd[f"head_layers.{i}.{hname}.0.bias"])
    return out


def draw_batchnorm_(sd: dict, g: torch.Generator) -> dict:
    """Re-draw every BatchNorm entry away from the identity: weight about 1, bias and running_mean O(0.3), running_var uniform in 0.5 .. 2."""
    for k in list(sd):
        if ".normalization." not in k:
            continue
        shape = sd[k].shape
        if k.endswith(".weight"):
            sd[k] = 1.0 + 0.3 * torch.randn(shape, generator=g)
        elif k.endswith(".bias") or k.endswith(".running_mean"):
            sd[k] = 0.3 * torch.randn(shape, generator=g)
        elif k.endswith(".running_var"):
            sd[k] = 0.5 + 1.5 * torch.rand(shape, generator=g)
    return sd


def init_state(shapes: Dict[str, tuple], buffers: Dict[str, torch.Tensor], seed: int) -> dict:
    """A random state dict over the given parameter shapes and buffers (``Model.param_shapes`` / ``Model.buffers``): He-scaled conv weights (the maps keep
    their scale through the ReLUs), small biases, BatchNorm entries from ``draw_batchnorm_``."""
    g = torch.Generator().manual_seed(seed)
    sd = {k: v.clone() for k, v in buffers.items()}
    for k, shape in shapes.items():
        if len(shape) > 1:
            fan_in = 1
            for d in shape[1:]:
                fan_in *= int(d)
            sd[k] = torch.randn(shape, generator=g) * math.sqrt(2.0 / fan_in)
        else:
            sd[k] = 0.1 * torch.randn(shape, generator=g)
    return draw_batchnorm_(sd, g)
