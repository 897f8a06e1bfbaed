"""CPU emulation of the Swin inference forward with fp16 STORAGE (the device's FMT_F16 plan, handle option ``swint_f16``).

A plain-torch Swin encoder-decoder forward from a ``tests.swin_ref.init_state_swint`` state dict in which every tensor
the device would keep in fp16 is rounded (``.half().float()``) at the point where a kernel stores it, and every weight
image of the fp16 matrix pipe likewise; all arithmetic stays fp32, as inside the kernels (fp32 accumulators, fp32
LayerNorm statistics, fp32 logits and softmax statistics, fp32 erf-GELU).  Rounding points:

* the patch stem output, every LayerNorm output and the patch-merge norm output;
* the qkv tensor; a padded token's q, k, v are ``half(qkv.bias)``;
* ``S = (q k^T) * 32^-0.5 + bias + mask`` stays fp32 (the scale goes on the fp32 product, not on q);
* ``p = half(exp(S - rowmax))``; ``o = (p v) / sum(p)`` with the sum over the ROUNDED p; o is stored in fp16;
* every Linear is ``linear(x, half(W), b)`` with an fp32 epilogue (bias, GELU, residual add) and an fp16 store --
  the residual stream is stored this way too;
* middle / decoder / head as tools/convnext_f16_emulation.py.

Three modes:

``fp32``       nothing is rounded: must equal ``tests.swin_ref.model_forward`` (tests/test_swint_f16_emulation_cpu.py)
``f16``        form (a): every activation, the residual stream included, and every matrix-pipe weight in fp16
``f16_res32``  form (b): as (a), but the residual stream (stem norm output, block and merge outputs) stays fp32

Run as a script it prints, for the configurations of tests/test_gpu_swint_f16.py plus Swin-tiny at 96 x 96 and Swin-small,
the worst head error of both forms against ``swin_ref``, normalised as the tests normalise it:
max |got - ref| / max(1, max |ref|).  The bar of the fp16 precision is 5e-3.
"""
from __future__ import annotations

import argparse
import os
import sys
from typing import Dict, Optional

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from oracle import cpu_ref as O  # noqa: E402
from tests import swin_ref as R  # noqa: E402

MODES = ("fp32", "f16", "f16_res32")
PFX = R.PFX
EPS = R.EPS
SMALL = {"embed": 32, "depths": [2, 2, 2, 2], "num_heads": [1, 2, 4, 8]}


def _h(t: torch.Tensor) -> torch.Tensor:
    return t.half().float()


def _band_mask(pH: int, pW: int, ws: int, sh) -> torch.Tensor:
    """torchvision's attention mask of a shifted block: (windows, N, N), 0 or -100."""
    m = torch.zeros((pH, pW))
    hs = ((0, -ws), (-ws, -sh[0]), (-sh[0], None))
    wsl = ((0, -ws), (-ws, -sh[1]), (-sh[1], None))
    c = 0
    for h in hs:
        for w in wsl:
            m[h[0]: h[1], w[0]: w[1]] = c
            c += 1
    nW = (pH // ws) * (pW // ws)
    m = m.view(pH // ws, ws, pW // ws, ws).permute(0, 2, 1, 3).reshape(nW, ws * ws)
    m = m.unsqueeze(1) - m.unsqueeze(2)
    return m.masked_fill(m != 0, -100.0).masked_fill(m == 0, 0.0)


def window_attention_core(qkv: torch.Tensor, qkv_bias: torch.Tensor, table: torch.Tensor, ws: int, heads: int, shift: int, act) -> torch.Tensor:
    """What window_attn(_f16)_kernel computes: the STORED (B, H, W, 3C) qkv map -> the stored (B, H, W, C) attention output (before proj).
    A padded token's q, k, v are the (stored-precision) bias: the reference pads the normed input with zeros in front of the Linear."""
    B, H, W, C3 = qkv.shape
    C = C3 // 3
    pr, pb = (ws - W % ws) % ws, (ws - H % ws) % ws
    pH, pW = H + pb, W + pr
    x = act(qkv_bias).expand(B, pH, pW, C3).clone()
    x[:, :H, :W] = qkv
    sh = [0 if ws >= pH else shift, 0 if ws >= pW else shift]
    if sum(sh) > 0:
        x = torch.roll(x, shifts=(-sh[0], -sh[1]), dims=(1, 2))
    nW = (pH // ws) * (pW // ws)
    N = ws * ws
    x = x.view(B, pH // ws, ws, pW // ws, ws, C3).permute(0, 1, 3, 2, 4, 5).reshape(B * nW, N, 3, heads, C // heads).permute(2, 0, 3, 1, 4)
    q, k, v = x[0], x[1], x[2]
    s = q.matmul(k.transpose(-2, -1)) * (C // heads) ** -0.5
    s = s + table[R.rel_index(ws)].view(N, N, -1).permute(2, 0, 1).unsqueeze(0)
    if sum(sh) > 0:
        s = (s.view(B, nW, heads, N, N) + _band_mask(pH, pW, ws, sh).unsqueeze(1).unsqueeze(0)).view(-1, heads, N, N)
    p = act(torch.exp(s - s.amax(dim=-1, keepdim=True)))
    o = act(p.matmul(v) / p.sum(dim=-1, keepdim=True))
    o = o.transpose(1, 2).reshape(B * nW, N, C)
    o = o.view(B, pH // ws, pW // ws, ws, ws, C).permute(0, 1, 3, 2, 4, 5).reshape(B, pH, pW, C)
    if sum(sh) > 0:
        o = torch.roll(o, shifts=(sh[0], sh[1]), dims=(1, 2))
    return o[:, :H, :W, :].contiguous()


def forward(sd: Dict[str, torch.Tensor], bb: dict, head_cfgs: dict, model_type: str, image: torch.Tensor, mode: str = "fp32",
            collect: Optional[dict] = None) -> Dict[str, torch.Tensor]:
    if mode not in MODES:
        raise ValueError(f"mode must be one of {MODES}")
    act = (lambda t: t) if mode == "fp32" else _h          # an activation slot
    res = act if mode != "f16_res32" else (lambda t: t)     # a slot of the residual stream
    wq = (lambda t: t) if mode == "fp32" else _h           # a weight image of the fp16 matrix pipe
    p = R.swin_plan(bb)
    tail = p["tail"]
    pad = tail["k"] // 2
    ws = p["ws"]
    x = O.normalize_input(image)
    cin = int(bb["in_channels"])
    if x.shape[-3] != cin:
        if x.shape[-3] == 1:
            x = x.repeat(1, 3, 1, 1)
        else:
            r, g, b = x.unbind(dim=-3)
            x = (0.2989 * r + 0.587 * g + 0.114 * b).unsqueeze(-3)

    def ln(t, n):  # statistics and affine in fp32 on the stored input
        return F.layer_norm(t, (t.shape[-1],), sd[n + ".weight"], sd[n + ".bias"], EPS)

    def put(name, t):
        if collect is not None:
            collect[name] = t.permute(0, 3, 1, 2)

    # stem: fp32 weights on the vector pipe, fp16 store; the LayerNorm reads the stored tensor and starts the residual stream
    x = act(F.conv2d(x, sd[f"{PFX}.0.0.weight"], sd[f"{PFX}.0.0.bias"], stride=p["stride"], padding=1)).permute(0, 2, 3, 1)
    x = res(ln(x, f"{PFX}.0.2"))
    put(f"{PFX}.0", x)
    enc_out = [x]
    fi = 1
    for si, (d, h) in enumerate(zip(p["depths"], p["heads"])):
        for j in range(d):
            n = f"{PFX}.{fi}.{j}"
            y = act(ln(x, n + ".norm1"))
            qkv = act(F.linear(y, wq(sd[n + ".attn.qkv.weight"]), sd[n + ".attn.qkv.bias"]))
            o = window_attention_core(qkv, sd[n + ".attn.qkv.bias"], sd[n + ".attn.relative_position_bias_table"], ws, h, 0 if j % 2 == 0 else ws // 2, act)
            x = res(F.linear(o, wq(sd[n + ".attn.proj.weight"]), sd[n + ".attn.proj.bias"]) + x)
            put(n + ".attn", x)
            y = act(ln(x, n + ".norm2"))
            y = act(F.gelu(F.linear(y, wq(sd[n + ".mlp.0.weight"]), sd[n + ".mlp.0.bias"])))
            x = res(F.linear(y, wq(sd[n + ".mlp.3.weight"]), sd[n + ".mlp.3.bias"]) + x)
            put(n, x)
        enc_out.append(x)
        fi += 1
        if si + 1 < len(p["depths"]):
            n = f"{PFX}.{fi}"
            H, W = x.shape[1:3]
            y = F.pad(x, (0, 0, 0, W % 2, 0, H % 2))
            y = torch.cat([y[:, 0::2, 0::2], y[:, 1::2, 0::2], y[:, 0::2, 1::2], y[:, 1::2, 1::2]], -1)
            y = act(ln(y, n + ".norm"))
            x = res(F.linear(y, wq(sd[n + ".reduction.weight"])))
            put(n, x)
            enc_out.append(x)
            fi += 1
    enc_out[-1] = act(ln(enc_out[-1], "backbone.enc.norm"))
    put("backbone.enc.norm", enc_out[-1])
    enc_out = [t.permute(0, 3, 1, 2) for t in enc_out]
    feats = [act(t) for t in enc_out[::2][::-1]]  # (a decoder conv reads its skip in fp16 either way)
    x = act(O.same_pool2(enc_out[-1]))
    for convs in tail["mid"]:
        for n, _, _ in convs:
            x = act(F.relu(F.conv2d(x, wq(sd[n + ".weight"]), sd[n + ".bias"], padding=pad)))
            if collect is not None:
                collect[n] = x
    middle = x
    outs, strides = [], []
    for i, blk in enumerate(tail["dec"]):
        if blk["interp"]:
            x = act(F.interpolate(x, scale_factor=2, mode="bilinear", align_corners=False))
        else:
            n, _, _ = blk["trans"]
            x = act(F.relu(F.conv_transpose2d(x, wq(sd[n + ".weight"]), sd[n + ".bias"], stride=2, padding=1, output_padding=1)))
        if i < len(feats) and blk.get("concat", True):
            x = torch.cat((feats[i], x), dim=1)
        for n, _, _ in blk["convs"]:
            x = act(F.relu(F.conv2d(x, wq(sd[n + ".weight"]), sd[n + ".bias"], padding=pad)))
            if collect is not None:
                collect[n] = x
        outs.append(x)
        strides.append(blk["stride"])
    out = {}
    for i, (hname, key) in enumerate(O.HEAD_ORDER[model_type]):
        hc = head_cfgs[key]
        if hname == "ClassVectorsHead":
            raise ValueError("class-vector heads stay on the exact path: nothing to emulate")
        feat = outs[strides.index(hc["output_stride"])] if outs else middle
        out[hname] = F.conv2d(feat, wq(sd[f"head_layers.{i}.{hname}.0.weight"]), sd[f"head_layers.{i}.{hname}.0.bias"])  # fp32 output
    return out


def _bb(**kw):
    bb = {"model_type": None, "arch": SMALL, "in_channels": 1, "patch_size": 4, "window_size": 7, "kernel_size": 3, "filters_rate": 2, "convs_per_block": 2,
          "up_interpolate": True, "stem_patch_stride": 2, "output_stride": 2, "max_stride": 32, "pre_trained_weights": None}
    bb.update(kw)
    return bb


def _heads(n, stride=2):
    return {"confmaps": {"part_names": [str(i) for i in range(n)], "sigma": 2.5, "output_stride": stride}}


def _u8(shape, seed):
    return torch.randint(0, 256, shape, dtype=torch.uint8, generator=torch.Generator().manual_seed(seed))


def cases():
    """(label, bb, heads, model_type, image, state seed): the configurations of tests/test_gpu_swint_f16.py (those of tests/test_gpu_swint.py,
    images and seeds included), then Swin-tiny at 96 x 96 and Swin-small."""
    tiny = _bb(model_type="tiny", arch=None, in_channels=3)
    small = _bb(model_type="small", arch=None, in_channels=3)
    return [
        ("SMALL w7 2x64x96 u8", _bb(), _heads(5), "single_instance", _u8((2, 1, 64, 96), 11), 7),
        ("SMALL w7 2x64x192 u8", _bb(), _heads(3), "single_instance", _u8((2, 1, 64, 192), 12), 8),
        ("SMALL w4 1x64x64 u8", _bb(window_size=4), _heads(3), "single_instance", _u8((1, 1, 64, 64), 14), 14),
        ("SMALL w8 1x64x64 u8", _bb(window_size=8), _heads(3), "single_instance", _u8((1, 1, 64, 64), 14), 18),
        ("tiny rgb 1x64x64", tiny, _heads(13), "centered_instance", torch.rand((1, 3, 64, 64), generator=torch.Generator().manual_seed(3)), 7),
        ("tiny rgb 1x96x96", tiny, _heads(13), "centered_instance", torch.rand((1, 3, 96, 96), generator=torch.Generator().manual_seed(3)), 7),
        ("small rgb 1x96x96", small, _heads(13), "centered_instance", torch.rand((1, 3, 96, 96), generator=torch.Generator().manual_seed(3)), 7),
    ]


def head_error(got: Dict[str, torch.Tensor], ref: Dict[str, torch.Tensor]) -> float:
    return max(float((got[k] - t).abs().max()) / max(1.0, float(t.abs().max())) for k, t in ref.items())


def worst_errors(case, modes=MODES) -> Dict[str, float]:
    _, bb, heads, mt, img, seed = case
    sd = R.init_state_swint(bb, heads, mt, seed=seed)
    ref = R.model_forward(sd, bb, heads, mt, img)
    return {mode: head_error(forward(sd, bb, heads, mt, img, mode), ref) for mode in modes}


def worst_block_error(case, mode: str = "f16") -> float:
    """Worst labelled block (``<block>.attn``, ``<block>``, merge outputs, norms) of one case, in units of max(1, scale)."""
    _, bb, heads, mt, img, seed = case
    sd = R.init_state_swint(bb, heads, mt, seed=seed)
    want, got = {}, {}
    R.model_forward(sd, bb, heads, mt, img, collect=want)
    forward(sd, bb, heads, mt, img, mode, collect=got)
    return max(float((got[k] - t).abs().max()) / max(1.0, float(t.abs().max())) for k, t in want.items() if k in got)


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--blocks", action="store_true", help="also print the worst labelled block of form (a)")
    a = ap.parse_args(argv)
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
    print(f"{'configuration':<24} {'fp32':>10} {'(a) f16':>10} {'(b) res32':>10}   (worst head error / max(1, max|ref|); bar 5e-3)")
    for case in cases():
        e = worst_errors(case)
        extra = f"   worst block (a) {worst_block_error(case):.2e}" if a.blocks else ""
        print(f"{case[0]:<24} {e['fp32']:>10.2e} {e['f16']:>10.2e} {e['f16_res32']:>10.2e}{extra}", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
