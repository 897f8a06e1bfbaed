"""Plain-torch restatement of the Swin Transformer wrapper (reference ``sleap_nn/architectures/swint.py``; the encoder
blocks are torchvision's ``SwinTransformerBlock`` / ``shifted_window_attention`` / ``PatchMerging``, version 1).

torchvision is not installed here, so this restates its public definition; tests/test_swint_cpu.py compares the
block and the patch merging with HuggingFace transformers' independent implementation (not a torchvision pin).
The pool / middle / decoder half reuses the oracle's ConvNeXt plan and ``decoder_forward``: the reference's two
wrappers share that code.
"""
import math
from typing import Dict, Optional

import torch
import torch.nn.functional as F

from oracle import cpu_ref as O

ARCHS = {
    "tiny": {"embed": 96, "depths": [2, 2, 6, 2], "num_heads": [3, 6, 12, 24]},
    "small": {"embed": 96, "depths": [2, 2, 18, 2], "num_heads": [3, 6, 12, 24]},
    "base": {"embed": 128, "depths": [2, 2, 18, 2], "num_heads": [4, 8, 16, 32]},
}
EPS = 1e-5
PFX = "backbone.enc.features"


def rel_index(ws: int) -> torch.Tensor:
    coords = torch.stack(torch.meshgrid(torch.arange(ws), torch.arange(ws), indexing="ij")).flatten(1)
    rel = (coords[:, :, None] - coords[:, None, :]).permute(1, 2, 0).contiguous()
    rel[:, :, 0] += ws - 1
    rel[:, :, 1] += ws - 1
    rel[:, :, 0] *= 2 * ws - 1
    return rel.sum(-1).flatten()


def window_attention(x, qkv_w, qkv_b, proj_w, proj_b, table, ws: int, heads: int, shift: int, index: Optional[torch.Tensor] = None):
    """torchvision ``shifted_window_attention`` on a (B, H, W, C) map, dropout 0."""
    B, H, W, C = x.shape
    pr, pb = (ws - W % ws) % ws, (ws - H % ws) % ws
    x = F.pad(x, (0, 0, 0, pr, 0, pb))
    _, pH, pW, _ = x.shape
    sh = [shift, shift]
    if ws >= pH:
        sh[0] = 0
    if ws >= pW:
        sh[1] = 0
    if sum(sh) > 0:
        x = torch.roll(x, shifts=(-sh[0], -sh[1]), dims=(1, 2))
    nW = (pH // ws) * (pW // ws)
    N = ws * ws
    x = x.view(B, pH // ws, ws, pW // ws, ws, C).permute(0, 1, 3, 2, 4, 5).reshape(B * nW, N, C)
    qkv = F.linear(x, qkv_w, qkv_b).reshape(x.size(0), N, 3, heads, C // heads).permute(2, 0, 3, 1, 4)
    q, k, v = qkv[0], qkv[1], qkv[2]
    q = q * (C // heads) ** -0.5
    attn = q.matmul(k.transpose(-2, -1))
    idx = rel_index(ws) if index is None else index
    attn = attn + table[idx].view(N, N, -1).permute(2, 0, 1).unsqueeze(0)
    if sum(sh) > 0:
        m = x.new_zeros((pH, pW))
        hs = ((0, -ws), (-ws, -sh[0]), (-sh[0], None))
        wsl = ((0, -ws), (-ws, -sh[1]), (-sh[1], None))
        c = 0
        for h in hs:
            for w in wsl:
                m[h[0] : h[1], w[0] : w[1]] = c
                c += 1
        m = m.view(pH // ws, ws, pW // ws, ws).permute(0, 2, 1, 3).reshape(nW, N)
        m = m.unsqueeze(1) - m.unsqueeze(2)
        m = m.masked_fill(m != 0, -100.0).masked_fill(m == 0, 0.0)
        attn = attn.view(x.size(0) // nW, nW, heads, N, N) + m.unsqueeze(1).unsqueeze(0)
        attn = attn.view(-1, heads, N, N)
    attn = F.softmax(attn, dim=-1)
    x = attn.matmul(v).transpose(1, 2).reshape(x.size(0), N, C)
    x = F.linear(x, proj_w, proj_b)
    x = x.view(B, pH // ws, pW // ws, ws, ws, C).permute(0, 1, 3, 2, 4, 5).reshape(B, pH, pW, C)
    if sum(sh) > 0:
        x = torch.roll(x, shifts=(sh[0], sh[1]), dims=(1, 2))
    return x[:, :H, :W, :].contiguous()


def swin_block(sd: Dict[str, torch.Tensor], n: str, x: torch.Tensor, ws: int, heads: int, shift: int, collect: Optional[dict] = None) -> torch.Tensor:
    """``SwinTransformerBlock.forward`` on (B, H, W, C), stochastic depth = identity."""
    C = x.shape[-1]
    y = F.layer_norm(x, (C,), sd[n + ".norm1.weight"], sd[n + ".norm1.bias"], EPS)
    x = x + window_attention(y, sd[n + ".attn.qkv.weight"], sd[n + ".attn.qkv.bias"], sd[n + ".attn.proj.weight"], sd[n + ".attn.proj.bias"],
                             sd[n + ".attn.relative_position_bias_table"], ws, heads, shift)
    if collect is not None:
        collect[n + ".attn"] = x.permute(0, 3, 1, 2)
    y = F.layer_norm(x, (C,), sd[n + ".norm2.weight"], sd[n + ".norm2.bias"], EPS)
    y = F.linear(F.gelu(F.linear(y, sd[n + ".mlp.0.weight"], sd[n + ".mlp.0.bias"])), sd[n + ".mlp.3.weight"], sd[n + ".mlp.3.bias"])
    return x + y


def patch_merging(x: torch.Tensor, norm_w, norm_b, red_w) -> torch.Tensor:
    """``PatchMerging.forward`` on (B, H, W, C): pad to even, four phases on the channels, LayerNorm(4C), Linear(4C, 2C, bias=False)."""
    H, W = x.shape[1:3]
    x = F.pad(x, (0, 0, 0, W % 2, 0, H % 2))
    x = torch.cat([x[:, 0::2, 0::2], x[:, 1::2, 0::2], x[:, 0::2, 1::2], x[:, 1::2, 1::2]], -1)
    return F.linear(F.layer_norm(x, (x.shape[-1],), norm_w, norm_b, EPS), red_w)


def arch_of(bb: dict) -> dict:
    mt = bb.get("model_type", None)
    return ARCHS[mt] if mt in ARCHS else (bb.get("arch", None) or ARCHS["tiny"])


def swin_plan(bb: dict) -> dict:
    """Encoder enumeration + the ConvNeXt wrapper's middle / decoder plan over the Swin stage widths."""
    a = arch_of(bb)
    embed, depths, heads = int(a["embed"]), [int(d) for d in a["depths"]], [int(h) for h in a["num_heads"]]
    channels = [embed * 2**i for i in range(len(depths))]
    tail = O.convnext_plan({**bb, "model_type": None, "arch": {"depths": depths, "channels": channels}, "stem_patch_kernel": int(bb.get("patch_size", 4))})
    return {"embed": embed, "depths": depths, "heads": heads, "channels": channels, "ws": int(bb.get("window_size", 7)), "patch": int(bb.get("patch_size", 4)),
            "stride": int(bb.get("stem_patch_stride", 2)), "cin": int(bb.get("in_channels", 1)), "tail": tail}


def init_state_swint(bb: dict, head_cfgs: dict, model_type: str, seed: int = 1234, head_scale: float = 1.0) -> Dict[str, torch.Tensor]:
    """Synthetic weights in the manner of ``oracle.cpu_ref.init_state_convnext(randomize_affine=True)``: xavier-uniform weights, perturbed biases and
    LayerNorm affines, the relative-position bias table N(0, 0.5) so that it matters; the index buffers included, as a checkpoint has them."""
    p = swin_plan(bb)
    g = torch.Generator().manual_seed(seed)
    sd: Dict[str, torch.Tensor] = {}

    def xavier(shape, fan_in, fan_out):
        return (torch.rand(shape, generator=g) * 2 - 1) * math.sqrt(6.0 / (fan_in + fan_out))

    def vec(n, base, spread):
        return torch.full((n,), float(base)) + (torch.rand(n, generator=g) * 2 - 1) * spread

    def norm(n, c):
        sd[n + ".weight"] = vec(c, 1.0, 0.3)
        sd[n + ".bias"] = vec(c, 0.0, 0.1)

    def linear(n, ci, co, bias=True):
        sd[n + ".weight"] = xavier((co, ci), ci, co)
        if bias:
            sd[n + ".bias"] = vec(co, 0.0, 0.1)

    E, kk, ws = p["embed"], p["patch"], p["ws"]
    sd[f"{PFX}.0.0.weight"] = xavier((E, p["cin"], kk, kk), p["cin"] * kk * kk, E * kk * kk)
    sd[f"{PFX}.0.0.bias"] = vec(E, 0.0, 0.1)
    norm(f"{PFX}.0.2", E)
    fi = 1
    for si, (d, c, h) in enumerate(zip(p["depths"], p["channels"], p["heads"])):
        for j in range(d):
            n = f"{PFX}.{fi}.{j}"
            norm(n + ".norm1", c)
            linear(n + ".attn.qkv", c, 3 * c)
            sd[n + ".attn.relative_position_bias_table"] = torch.randn(((2 * ws - 1) ** 2, h), generator=g) * 0.5
            sd[n + ".attn.relative_position_index"] = rel_index(ws)
            linear(n + ".attn.proj", c, c)
            norm(n + ".norm2", c)
            linear(n + ".mlp.0", c, 4 * c)
            linear(n + ".mlp.3", 4 * c, c)
        fi += 1
        if si + 1 < len(p["channels"]):
            n = f"{PFX}.{fi}"
            linear(n + ".reduction", 4 * c, 2 * c, bias=False)
            norm(n + ".norm", 4 * c)
            fi += 1
    norm("backbone.enc.norm", p["channels"][-1])
    tail = p["tail"]
    k = tail["k"]
    for convs in tail["mid"]:
        for n, ci, co in convs:
            sd[n + ".weight"] = xavier((co, ci, k, k), ci * k * k, co * k * k)
            sd[n + ".bias"] = vec(co, 0.0, 0.05)
    for blk in tail["dec"]:
        if not blk["interp"]:
            n, ci, co = blk["trans"]
            sd[n + ".weight"] = xavier((ci, co, 3, 3), co * 9, ci * 9)
            sd[n + ".bias"] = vec(co, 0.0, 0.05)
        for n, ci, co in blk["convs"]:
            sd[n + ".weight"] = xavier((co, ci, k, k), ci * k * k, co * k * k)
            sd[n + ".bias"] = vec(co, 0.0, 0.05)
    for i, (hname, key) in enumerate(O.HEAD_ORDER[model_type]):
        hc = head_cfgs[key]
        ci = tail["stride_to_filters"][hc["output_stride"]]
        co = O.head_channels(hname, hc)
        sd[f"head_layers.{i}.{hname}.0.weight"] = xavier((co, ci, 1, 1), ci, co) * head_scale
        sd[f"head_layers.{i}.{hname}.0.bias"] = torch.zeros(co)
    return sd


def swint_forward(sd: Dict[str, torch.Tensor], bb: dict, x: torch.Tensor, collect: Optional[dict] = None) -> dict:
    """``SwinTWrapper.forward`` (swint.py:376-400) over ``SwinTransformerEncoder.forward`` (:148-163).  ``x``: normalised (B, C, H, W)."""
    p = swin_plan(bb)
    tail = p["tail"]
    pad = tail["k"] // 2
    ws = p["ws"]
    x = F.conv2d(x, sd[f"{PFX}.0.0.weight"], sd[f"{PFX}.0.0.bias"], stride=p["stride"], padding=1).permute(0, 2, 3, 1)
    x = F.layer_norm(x, (x.shape[-1],), sd[f"{PFX}.0.2.weight"], sd[f"{PFX}.0.2.bias"], EPS)
    enc_out = [x]
    if collect is not None:
        collect[f"{PFX}.0"] = x.permute(0, 3, 1, 2)
    fi = 1
    for si, (d, h) in enumerate(zip(p["depths"], p["heads"])):
        for j in range(d):
            n = f"{PFX}.{fi}.{j}"
            x = swin_block(sd, n, x, ws, h, 0 if j % 2 == 0 else ws // 2, collect)
            if collect is not None:
                collect[n] = x.permute(0, 3, 1, 2)
        enc_out.append(x)
        fi += 1
        if si + 1 < len(p["depths"]):
            n = f"{PFX}.{fi}"
            x = patch_merging(x, sd[n + ".norm.weight"], sd[n + ".norm.bias"], sd[n + ".reduction.weight"])
            if collect is not None:
                collect[n] = x.permute(0, 3, 1, 2)
            enc_out.append(x)
            fi += 1
    enc_out[-1] = F.layer_norm(enc_out[-1], (enc_out[-1].shape[-1],), sd["backbone.enc.norm.weight"], sd["backbone.enc.norm.bias"], EPS)
    if collect is not None:
        collect["backbone.enc.norm"] = enc_out[-1].permute(0, 3, 1, 2)
    enc_out = [t.permute(0, 3, 1, 2) for t in enc_out]
    feats = enc_out[::2][::-1]
    x = O.same_pool2(enc_out[-1])
    for convs in tail["mid"]:
        for n, _, _ in convs:
            x = F.relu(F.conv2d(x, sd[n + ".weight"], sd[n + ".bias"], padding=pad))
            if collect is not None:
                collect[n] = x
    middle = x
    outs, strides = O.decoder_forward(sd, tail, x, feats, collect)
    return {"outputs": outs, "strides": strides, "middle_output": middle}


def model_forward(sd, bb: dict, head_cfgs: dict, model_type: str, image: torch.Tensor, collect: Optional[dict] = None) -> Dict[str, torch.Tensor]:
    """``oracle.cpu_ref.model_forward`` with the Swin backbone (confidence-map / PAF / offset heads: plain 1x1 convolutions)."""
    x = O.normalize_input(image)
    cin = int(bb["in_channels"])
    if x.shape[-3] != cin:
        if x.shape[-3] == 1:
            x = x.repeat(1, 3, 1, 1)
        else:
            r, g, b = x.unbind(dim=-3)
            x = (0.2989 * r + 0.587 * g + 0.114 * b).unsqueeze(-3)
    bo = swint_forward(sd, bb, x, collect)
    out = {}
    for i, (hname, key) in enumerate(O.HEAD_ORDER[model_type]):
        hc = head_cfgs[key]
        feat = bo["outputs"][bo["strides"].index(hc["output_stride"])]
        out[hname] = F.conv2d(feat, sd[f"head_layers.{i}.{hname}.0.weight"], sd[f"head_layers.{i}.{hname}.0.bias"])
    return out
