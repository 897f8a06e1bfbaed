"""The ResNet-50 (``pretrained`` backbone, HuggingFace ResNetBackbone) inference forward at cfg4's shape (centered-instance, 64 crops of 384 x 384, exact fp32),
split by op group.

    python tools/resnet_timing.py [--batch 64] [--size 384] [--forwards 20] [--repeats 3] [--out profiles/resnet_timing.json]

In the form of tools/convnextv2_timing.py: each timed loop is `--forwards` forwards, every forward between two device events, behind untimed warm-up calls (at
least three, and at least benchlegs.common.WARM_MS of wall time); `--repeats` loops per leg, the legs alternating (ResNet-50, ConvNeXtV2-nano).  Reported: the
median forward of every repeat and the spread between those medians (max - min).  Untimed passes then take the per-op split from ph_model_set_profiling (HIP events
around every op), grouped into stem (7x7 conv + max pool), 1x1 convs (row GEMMs), 3x3 stride-1 convs, strided convs, element-wise, decoder, head; for the two
row-GEMM groups and the stem, the executed TFLOP/s against the fp32 MFMA peak.  The backbone did not run before: there is no earlier time to compare with, and the
ConvNeXtV2-nano forward re-measured in the same process is context only (another network).  The decoder settings are the defaults the reference's sample
``pretrained`` config leaves in place (docs/guides/pretrained-backbones.md sets output_stride 2 and max_stride 32 only).  Needs an MI355X: there is no CPU path.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from benchlegs.common import CFG4_HEADS, MFMA_F32_PEAK_TFLOPS  # noqa: E402
from convnextv2_timing import NANO_BB, _summary, _timed, _warm  # noqa: E402
from sleap_nn_amd import _lib as L  # noqa: E402
from sleap_nn_amd.architectures.model import Model  # noqa: E402

RESNET_BB = dict(NANO_BB, model_name="microsoft/resnet-50", allow_resnet=True)
STEM, GEMM1, CONV3, STRIDED, ELT, DEC, HEAD = ("stem (7x7/s2 conv + 3x3/s2 max pool)", "1x1 convs (row GEMM; bottleneck tails with residual + ReLU)", "3x3 stride-1 convs",
                                               "strided convs (3x3/s2, 1x1/s2 row GEMMs)", "element-wise (add + ReLU)", "decoder (bilinear x2, conv3x3)", "head")


def _group(op) -> str:
    enc = (op.label or "").startswith("backbone.enc.")
    if op.kind == L.OP_RESNET_STEM:
        return STEM
    if op.kind == L.OP_CONV_S2:
        return STRIDED
    if op.kind == L.OP_ADD_RELU:
        return ELT
    if op.kind == L.OP_LINEAR and enc:
        return GEMM1
    if op.kind == L.OP_CONV and enc:
        return CONV3
    return HEAD if op.kind == L.OP_HEAD else DEC


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--size", type=int, default=384)
    ap.add_argument("--forwards", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resnet_timing.json"))
    a = ap.parse_args(argv)
    if a.forwards < 20 or a.repeats < 3:
        ap.error("at least 20 forwards per loop and 3 repeats")
    if not torch.cuda.is_available():
        raise SystemExit("resnet_timing needs an MI355X (no CPU path)")
    dev = torch.device("cuda", 0)
    rgb = torch.randint(0, 256, (a.batch, 3, a.size, a.size), dtype=torch.uint8, generator=torch.Generator().manual_seed(4321)).to(dev)
    rn = Model("pretrained", RESNET_BB, CFG4_HEADS, "centered_instance").init_xavier_(seed=1234, head_scale=0.05).to(dev)
    v2 = Model("pretrained", NANO_BB, CFG4_HEADS, "centered_instance").init_xavier_(seed=1234, head_scale=0.05).to(dev)
    f_rn = lambda: rn(rgb)  # noqa: E731
    f_v2 = lambda: v2(rgb)  # noqa: E731
    med = {"rn": [], "v2": []}
    for _ in range(a.repeats):  # the legs alternate, so that a drift of the machine lands on both
        for key, fn in (("rn", f_rn), ("v2", f_v2)):
            _warm(fn)
            med[key].append(statistics.median(_timed(fn, a.forwards)))
    out = f_rn()
    torch.cuda.synchronize()
    rn.set_profiling(True)
    for _ in range(5):
        f_rn()
    torch.cuda.synchronize()
    op_ms, n_fw = rn.read_profile()
    rn.set_profiling(False)
    table = rn.op_table(a.batch, a.size, a.size)
    ms, flops = {}, {}
    for op, t, r in zip(rn.ops, op_ms, table):
        ms[_group(op)] = ms.get(_group(op), 0.0) + t / max(n_fw, 1)
        flops[_group(op)] = flops.get(_group(op), 0.0) + r["flops"]
    rate = {k: {"direct_gflop": round(flops[k] / 1e9, 1), "tflops": round(flops[k] / (ms[k] * 1e-3) / 1e12, 1),
                "share_of_fp32_mfma_peak": round(flops[k] / (ms[k] * 1e-3) / 1e12 / MFMA_F32_PEAK_TFLOPS, 3)} for k in (STEM, GEMM1, STRIDED) if ms.get(k, 0.0) > 0}
    res = {"workload": f"ResNet-50 (pretrained backbone, HuggingFace ResNetBackbone, BatchNorm folded) centered-instance inference forward, {a.batch} crops of {a.size} x {a.size}, 13 nodes, "
                       "output stride 2, exact fp32",
           "backbone_config": RESNET_BB, "forwards_per_loop": a.forwards, "repeats": a.repeats, "outputs_finite": all(bool(torch.isfinite(v).all()) for v in out.values()),
           "parameters": rn.num_parameters(), "direct_tflop_per_forward": round(sum(r["flops"] for r in table) / 1e12, 3), "workspace_gbytes": round(rn._workspace.numel() / 1e9, 2),
           **_summary(med["rn"]),
           "per_op_ms": {k: round(v, 3) for k, v in sorted(ms.items(), key=lambda kv: -kv[1])},
           "share_of_forward": {k: round(v / sum(ms.values()), 4) for k, v in sorted(ms.items(), key=lambda kv: -kv[1])},
           "matrix_groups": rate, "fp32_mfma_peak_tflops": MFMA_F32_PEAK_TFLOPS,
           "convnextv2_nano_same_process": {"workload": "ConvNeXtV2-nano exact forward at the same shape; context only, another network, not a baseline", **_summary(med["v2"])}}
    print("| op group | ms | share |\n|---|---|---|")
    for k, v in res["per_op_ms"].items():
        print(f"| {k} | {v:.2f} | {100 * res['share_of_forward'][k]:.1f} % |")
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
