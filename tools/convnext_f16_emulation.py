"""CPU emulation of the ConvNeXt inference forward with fp16 STORAGE (the device's FMT_F16 plan).

A plain-torch ConvNeXt encoder-decoder forward from an ``oracle.cpu_ref.init_state_convnext`` state dict in
which every tensor the device would keep in fp16 is rounded (``.half().float()``) at the point where a kernel
stores it; all arithmetic stays fp32, as inside the kernels (fp32 accumulators, fp32 LayerNorm statistics,
fp32 erf-GELU).  Three modes:

``fp32``       nothing is rounded: must equal ``oracle.cpu_ref.model_forward`` (tests/test_convnext_f16_emulation_cpu.py)
``f16``        form (a): every activation, the CNBlock residual stream included, and every matrix-pipe weight in fp16
``f16_res32``  form (b): as (a), but the residual stream (stem LayerNorm output, block outputs) stays fp32

Run as a script it prints, for the four configurations of tests/test_gpu_convnext.py::test_convnext_forward_matches_oracle
and ConvNeXt-tiny on a 96 x 96 crop, the worst head error of both forms against the fp32 oracle, normalised as the
tests normalise it: max |got - ref| / max(1, max |ref|).  The bar of the fp16 precision is 5e-3.
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

MODES = ("fp32", "f16", "f16_res32")


def _h(t: torch.Tensor) -> torch.Tensor:
    return t.half().float()


def forward(sd: Dict[str, torch.Tensor], bb: dict, head_cfgs: dict, model_type: str, image: torch.Tensor, mode: str = "fp32",
            collect: Optional[dict] = None) -> Dict[str, torch.Tensor]:
    if mode not in MODES:
        raise ValueError(f"mode must be one of {MODES}")
    act = (lambda t: t) if mode == "fp32" else _h          # an activation slot
    res = act if mode != "f16_res32" else (lambda t: t)     # a slot of the residual stream
    wq = (lambda t: t) if mode == "fp32" else _h           # a weight image of the fp16 matrix pipe
    plan = O.convnext_plan(bb)
    pad = plan["k"] // 2
    x = O.normalize_input(image)
    cin = int(bb["in_channels"])
    if x.shape[-3] != cin:
        if x.shape[-3] == 1:
            x = x.repeat(1, 3, 1, 1)
        else:
            r, g, b = x.unbind(dim=-3)
            x = (0.2989 * r + 0.587 * g + 0.114 * b).unsqueeze(-3)

    def ln(t, w, b):  # statistics and affine in fp32 on the stored input
        return F.layer_norm(t.permute(0, 2, 3, 1), (t.shape[1],), w, b, O.LN_EPS).permute(0, 3, 1, 2)

    enc_out = []
    for e in plan["enc"]:
        n = e.get("name")
        if e["kind"] == "stem":  # fp32 weights on the vector pipe, fp16 store; LayerNorm reads the stored tensor
            x = act(F.conv2d(x, sd[n + ".0.weight"], sd[n + ".0.bias"], stride=e["stride"], padding=1))
            x = res(ln(x, sd[n + ".1.weight"], sd[n + ".1.bias"]))
        elif e["kind"] == "stage":
            for bn in e["blocks"]:
                c = x.shape[1]
                y = act(F.conv2d(x, sd[bn + ".block.0.weight"], sd[bn + ".block.0.bias"], padding=3, groups=c))  # (the keep-activations plan stores it; the fused kernel does not)
                y = act(ln(y, sd[bn + ".block.2.weight"], sd[bn + ".block.2.bias"])).permute(0, 2, 3, 1)
                y = act(F.gelu(F.linear(y, wq(sd[bn + ".block.3.weight"]), sd[bn + ".block.3.bias"])))
                y = F.linear(y, wq(sd[bn + ".block.5.weight"]), sd[bn + ".block.5.bias"]).permute(0, 3, 1, 2)
                x = res(sd[bn + ".layer_scale"] * y + x)
                if collect is not None:
                    collect[bn] = x
        else:
            x = act(ln(x, sd[n + ".0.weight"], sd[n + ".0.bias"]))
            x = res(F.conv2d(x, wq(sd[n + ".1.weight"]), sd[n + ".1.bias"], stride=2))
        if collect is not None and e["kind"] != "stage":
            collect[n] = x
        enc_out.append(x)
    feats = [act(t) for t in enc_out[::2][::-1]]  # (a decoder conv reads its skip in fp16 either way: form (b) converts in its loader)
    x = act(O.same_pool2(enc_out[-1]))
    for convs in plan["mid"]:
        for n, _, _ in convs:
            x = act(F.relu(F.conv2d(x, wq(sd[n + ".weight"]), sd[n + ".bias"], padding=pad)))
            if collect is not None:
                collect[n] = x
    middle = x
    outs, strides = [], []
    for i, blk in enumerate(plan["dec"]):
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
        y = F.conv2d(feat, wq(sd[f"head_layers.{i}.{hname}.0.weight"]), sd[f"head_layers.{i}.{hname}.0.bias"])  # fp32 output
        out[hname] = torch.sigmoid(y) if hname == "ClassMapsHead" else y
    return out


def _bb(**kw):
    bb = {"model_type": None, "arch": None, "in_channels": 1, "kernel_size": 3, "filters_rate": 2, "convs_per_block": 2, "up_interpolate": True,
          "stem_patch_kernel": 4, "stem_patch_stride": 2, "output_stride": 2, "max_stride": 32}
    bb.update(kw)
    return bb


def _heads(n, stride):
    return {"confmaps": {"part_names": [str(i) for i in range(n)], "sigma": 2.5, "output_stride": stride}}


def cases():
    """(label, bb, heads, model_type, image, seed, layer_scale): the GPU tests' own configurations."""
    out = []
    for channels, depths, ss, os_, hw, batch in [
        ([16, 32, 64, 128], [1, 2, 1, 1], 2, 2, (64, 96), 2),
        ([24, 40, 72, 136], [2, 1, 1, 1], 2, 4, (64, 64), 3),
        ([32, 64, 128, 256], [1, 1, 2, 1], 4, 1, (128, 64), 1),
        ([96, 192, 384, 768], [1, 1, 1, 1], 2, 2, (96, 160), 2),
    ]:
        g = torch.Generator().manual_seed(11)
        img = torch.randint(0, 256, (batch, 1, hw[0], hw[1]), dtype=torch.uint8, generator=g)
        bb = _bb(arch={"depths": depths, "channels": channels}, stem_patch_stride=ss, output_stride=os_)
        out.append((f"{channels[0]}-{channels[-1]} {hw[0]}x{hw[1]}x{batch}", bb, _heads(5, os_), "single_instance", img, 7, 0.5))
    g = torch.Generator().manual_seed(3)
    out.append(("tiny 96x96x1", _bb(model_type="tiny", in_channels=3, output_stride=2), _heads(13, 2), "centered_instance", torch.rand((1, 3, 96, 96), generator=g), 7, 0.3))
    return out


def worst_errors(case) -> Dict[str, float]:
    _, bb, heads, mt, img, seed, ls = case
    sd = O.init_state_convnext(bb, heads, mt, seed=seed, head_scale=1.0, layer_scale=ls, randomize_affine=True)
    ref = O.model_forward(sd, bb, heads, mt, img, backbone="convnext")
    res = {}
    for mode in MODES:
        got = forward(sd, bb, heads, mt, img, mode)
        res[mode] = max(float((got[k] - t).abs().max()) / max(1.0, float(t.abs().max())) for k, t in ref.items())
    return res


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.parse_args(argv)
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
    print(f"{'configuration':<24} {'fp32':>10} {'(a) f16':>10} {'(b) res32':>10}   (worst head error / max(1, max|ref|); bar 5e-3)")
    for case in cases():
        e = worst_errors(case)
        print(f"{case[0]:<24} {e['fp32']:>10.2e} {e['f16']:>10.2e} {e['f16_res32']:>10.2e}", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
