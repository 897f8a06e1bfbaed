"""The Swinv2-tiny (``pretrained`` backbone, HuggingFace Swinv2Backbone, microsoft/swinv2-tiny-patch4-window8-256) inference forward at cfg4's shape (centered-instance,
64 crops of 384 x 384, exact fp32), split by op group.

    python tools/swinv2_timing.py [--batch 64] [--size 384] [--forwards 20] [--repeats 3] [--out profiles/swinv2_timing.json]

In the form of tools/resnet_timing.py: each timed loop is `--forwards` forwards, every forward between two device events, behind untimed warm-up calls (at least three,
and at least benchlegs.common.WARM_MS of wall time); `--repeats` loops per leg, the legs alternating (Swinv2-tiny, Swin-tiny v1).  Reported: the median forward of every
repeat and the spread between those medians (max - min).  Untimed passes then take the per-op split from ph_model_set_profiling (HIP events around every op), grouped into
qkv / proj / MLP row GEMMs, cosine window attention, post-norms (residual-after-norm LayerNorm), patch merging (gather, reduction GEMM, norm), stem, decoder, head.  For
the attention kernel alone: the FLOPs it executes (full 32-token MFMA tiles; at window 8 both tiles are full) against the fp32 matrix peak, and its algorithmic bytes
(qkv read once, output written once) against 8 TB/s.  The backbone did not run before: there is no earlier time to compare with, and the Swin-tiny v1 forward measured
in the same process is context only (another network, one-channel input, window 7).  The weights are ``init_xavier_``'s (timing does not depend on them); the decoder
settings are those of tools/convnextv2_timing.py.  Needs an MI355X: there is no CPU path.
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
from convnextv2_timing import HBM_TBPS, NANO_BB, _summary, _timed, _warm  # noqa: E402
from sleap_nn_amd import _lib as L  # noqa: E402
from sleap_nn_amd.architectures.model import Model  # noqa: E402
from swint_timing import SWINT_BB  # noqa: E402

SWINV2_BB = dict(NANO_BB, model_name="microsoft/swinv2-tiny-patch4-window8-256", allow_swinv2=True)
ATT, QKV, PROJ, MLP, NORM, MERGE, STEM, DEC, HEAD = ("cosine window attention", "qkv GEMM", "proj GEMM", "MLP GEMMs (GELU)", "post-norms (shortcut + LayerNorm)",
                                                     "patch merging (gather, reduction GEMM, norm)", "stem (normalised patch conv + LayerNorm)", "decoder (bilinear x2, conv3x3)", "head")


def _group(op) -> str:
    label = op.label or ""
    if op.kind == L.OP_WINDOW_ATTN_V2:
        return ATT
    if op.kind == L.OP_PATCH_MERGE or ".downsample." in label:
        return MERGE
    if op.kind == L.OP_PATCH_STEM or label.endswith("embeddings.norm"):
        return STEM
    if op.kind == L.OP_LAYERNORM:
        return NORM
    if op.kind == L.OP_LINEAR and label.startswith("backbone.enc."):
        return QKV if label.endswith(".qkv") else PROJ if label.endswith("attention.output.dense") else MLP
    return HEAD if op.kind == L.OP_HEAD else DEC


def attention_executed_flops(model, batch: int, size: int) -> float:
    """What window_attn_v2_kernel issues: per (window, head) T x T tiles of 16 MFMAs for k q^T and T x 16 T for v^T p^T, T = ceil(N / 32), 4096 FLOPs per v_mfma_f32_32x32x2_f32."""
    total = 0.0
    for op, row in zip(model.ops, model.op_table(batch, size, size)):
        if op.kind != L.OP_WINDOW_ATTN_V2:
            continue
        h, w = row["out_hw"]
        ws, t = op.ksize, (op.ksize * op.ksize + 31) // 32
        total += batch * ((h + ws - 1) // ws) * ((w + ws - 1) // ws) * op.cin1 * (16 * t * t + 16 * t * t) * 4096.0
    return total


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--size", type=int, default=384)
    ap.add_argument("--forwards", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "swinv2_timing.json"))
    a = ap.parse_args(argv)
    if a.forwards < 20 or a.repeats < 3:
        ap.error("at least 20 forwards per loop and 3 repeats")
    if not torch.cuda.is_available():
        raise SystemExit("swinv2_timing needs an MI355X (no CPU path)")
    dev = torch.device("cuda", 0)
    gen = torch.Generator().manual_seed(4321)
    rgb = torch.randint(0, 256, (a.batch, 3, a.size, a.size), dtype=torch.uint8, generator=gen).to(dev)
    gray = torch.randint(0, 256, (a.batch, 1, a.size, a.size), dtype=torch.uint8, generator=gen).to(dev)
    v2 = Model("pretrained", SWINV2_BB, CFG4_HEADS, "centered_instance").init_xavier_(seed=1234, head_scale=0.05).to(dev)
    v1 = Model("swint", SWINT_BB, CFG4_HEADS, "centered_instance").init_xavier_(seed=1234, head_scale=0.05).to(dev)
    f_v2 = lambda: v2(rgb)  # noqa: E731
    f_v1 = lambda: v1(gray)  # noqa: E731
    med = {"v2": [], "v1": []}
    for _ in range(a.repeats):  # the legs alternate, so that a drift of the machine lands on both
        for key, fn in (("v2", f_v2), ("v1", f_v1)):
            _warm(fn)
            med[key].append(statistics.median(_timed(fn, a.forwards)))
    out = f_v2()
    torch.cuda.synchronize()
    v2.set_profiling(True)
    for _ in range(5):
        f_v2()
    torch.cuda.synchronize()
    op_ms, n_fw = v2.read_profile()
    v2.set_profiling(False)
    table = v2.op_table(a.batch, a.size, a.size)
    ms, flops = {}, {}
    for op, t, r in zip(v2.ops, op_ms, table):
        ms[_group(op)] = ms.get(_group(op), 0.0) + t / max(n_fw, 1)
        flops[_group(op)] = flops.get(_group(op), 0.0) + r["flops"]
    rate = {k: {"direct_gflop": round(flops[k] / 1e9, 1), "tflops": round(flops[k] / (ms[k] * 1e-3) / 1e12, 1),
                "share_of_fp32_mfma_peak": round(flops[k] / (ms[k] * 1e-3) / 1e12 / MFMA_F32_PEAK_TFLOPS, 3)} for k in (QKV, PROJ, MLP) if ms.get(k, 0.0) > 0}
    att_ms = ms.get(ATT, 0.0)
    att_bytes = sum(r["bytes"] for o, r in zip(v2.ops, table) if o.kind == L.OP_WINDOW_ATTN_V2)
    att_exec = attention_executed_flops(v2, a.batch, a.size)
    res = {"workload": f"Swinv2-tiny (pretrained backbone, HuggingFace Swinv2Backbone, window 8, image_size 256) centered-instance inference forward, {a.batch} crops of "
                       f"{a.size} x {a.size}, 13 nodes, output stride 2, exact fp32",
           "backbone_config": SWINV2_BB, "forwards_per_loop": a.forwards, "repeats": a.repeats, "outputs_finite": all(bool(torch.isfinite(v).all()) for v in out.values()),
           "parameters": v2.num_parameters(), "direct_tflop_per_forward": round(sum(r["flops"] for r in table) / 1e12, 3), "workspace_gbytes": round(v2._workspace.numel() / 1e9, 2),
           **_summary(med["v2"]),
           "per_op_ms": {k: round(v, 3) for k, v in sorted(ms.items(), key=lambda kv: -kv[1])},
           "share_of_forward": {k: round(v / sum(ms.values()), 4) for k, v in sorted(ms.items(), key=lambda kv: -kv[1])},
           "matrix_groups": rate, "fp32_mfma_peak_tflops": MFMA_F32_PEAK_TFLOPS,
           "cosine_window_attention": {"ms": round(att_ms, 3), "algorithmic_gflop": round(flops.get(ATT, 0.0) / 1e9, 2), "executed_gflop": round(att_exec / 1e9, 2),
                                       "executed_tflops": round(att_exec / (att_ms * 1e-3) / 1e12, 2) if att_ms > 0 else None,
                                       "share_of_fp32_matrix_peak": round(att_exec / (att_ms * 1e-3) / 1e12 / MFMA_F32_PEAK_TFLOPS, 4) if att_ms > 0 else None,
                                       "algorithmic_gbytes": round(att_bytes / 1e9, 3),
                                       "share_of_8_tbps": round(att_bytes / (att_ms * 1e-3) / 1e12 / HBM_TBPS, 4) if att_ms > 0 else None},
           "swin_tiny_v1_same_process": {"workload": "Swin-tiny v1 (swint backbone, one-channel input, window 7) exact forward at the same shape; context only, another network, not a baseline",
                                         **_summary(med["v1"])},
           "not_measured": "kernel times from a profiler trace, any other batch or frame size, the small / base sizes"}
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
