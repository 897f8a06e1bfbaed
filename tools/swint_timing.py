"""The Swin-tiny inference forward at cfg4's shape (centered-instance, 64 crops of 384 x 384, exact fp32), split by op kind.

    python tools/swint_timing.py [--batch 64] [--size 384] [--forwards 20] [--repeats 3] [--out result.json]

Each timed loop is `--forwards` forwards, every forward between two device events, behind untimed warm-up calls (at least three, and at
least benchlegs.common.WARM_MS of wall time); `--repeats` loops.  Reported: the median forward of every repeat and the spread between those
medians (max - min).  A last, untimed pass takes the per-op split from ph_model_set_profiling (HIP events around every op), grouped into
qkv / proj / MLP row GEMMs, window attention, layer norms, patch merging, stem, middle + decoder, head.  For the attention kernel alone: the
FLOPs it executes (full 32-token MFMA tiles, dead rows and columns included) against the fp32 matrix peak, and its algorithmic bytes (qkv
read once, output written once) against 8 TB/s.  Needs an MI355X: there is no CPU path.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from benchlegs.common import CFG4_HEADS, MFMA_F32_PEAK_TFLOPS, WARM_MS  # noqa: E402
from sleap_nn_amd import _lib as L  # noqa: E402
from sleap_nn_amd.architectures.model import Model  # noqa: E402

SWINT_BB = {"in_channels": 1, "model_type": "tiny", "arch": None, "patch_size": 4, "stem_patch_stride": 2, "window_size": 7, "kernel_size": 3, "filters_rate": 2,
            "convs_per_block": 2, "up_interpolate": True, "output_stride": 2, "max_stride": 32}
HBM_TBPS = 8.0


def _group(op) -> str:
    if op.kind == L.OP_WINDOW_ATTN:
        return "window attention"
    if op.kind == L.OP_LAYERNORM:
        return "layer norms"
    if op.kind == L.OP_PATCH_MERGE or (op.kind == L.OP_LINEAR and op.label.endswith(".reduction")):
        return "patch merging (gather + norm, reduction GEMM)"
    if op.kind == L.OP_LINEAR:
        leaf = op.label.rsplit(".", 2)
        return {"qkv": "qkv GEMM", "proj": "proj GEMM (+ residual)"}.get(leaf[-1], "MLP GEMMs (GELU, + residual)")
    if op.kind == L.OP_PATCH_STEM:
        return "patch stem"
    if op.kind == L.OP_HEAD:
        return "head"
    return "middle + decoder (pool, conv3x3, bilinear x2)"


def _warm(fn):
    t0, k = time.perf_counter(), 0
    while k < 3 or 1e3 * (time.perf_counter() - t0) < WARM_MS:
        fn()
        k += 1
    torch.cuda.synchronize()


def _timed(fn, n):
    marks = [torch.cuda.Event(enable_timing=True) for _ in range(n + 1)]
    marks[0].record()
    for i in range(n):
        fn()
        marks[i + 1].record()
    torch.cuda.synchronize()
    return [marks[i].elapsed_time(marks[i + 1]) for i in range(n)]


def attention_executed_flops(model, batch: int, size: int) -> float:
    """What window_attn_kernel issues: per (window, head) T x T tiles of 16 MFMAs for q k^T and T x 16 T for p v, T = ceil(N / 32), 4096 FLOPs per v_mfma_f32_32x32x2_f32."""
    total = 0.0
    for op, row in zip(model.ops, model.op_table(batch, size, size)):
        if op.kind != L.OP_WINDOW_ATTN:
            continue
        h, w = row["out_hw"]
        ws, t = op.ksize, (op.ksize * op.ksize + 31) // 32
        windows = batch * ((h + ws - 1) // ws) * ((w + ws - 1) // ws)
        total += windows * op.cin1 * (16 * t * t + 16 * t * t) * 4096.0
    return total


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--size", type=int, default=384)
    ap.add_argument("--forwards", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    if a.forwards < 20 or a.repeats < 3:
        ap.error("at least 20 forwards per loop and 3 repeats")
    if not torch.cuda.is_available():
        raise SystemExit("swint_timing needs an MI355X (no CPU path)")
    dev = torch.device("cuda", 0)
    crops = torch.randint(0, 256, (a.batch, 1, a.size, a.size), dtype=torch.uint8, generator=torch.Generator().manual_seed(4321)).to(dev)
    m = Model("swint", SWINT_BB, CFG4_HEADS, "centered_instance").init_xavier_(seed=1234, head_scale=0.05).to(dev)
    fn = lambda: m(crops)  # noqa: E731
    medians = []
    for _ in range(a.repeats):
        _warm(fn)
        medians.append(statistics.median(_timed(fn, a.forwards)))
    out = fn()
    torch.cuda.synchronize()
    finite = all(bool(torch.isfinite(v).all()) for v in out.values())
    m.set_profiling(True)
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    op_ms, n_fw = m.read_profile()
    m.set_profiling(False)
    groups = {}
    for op, ms in zip(m.ops, op_ms):
        groups[_group(op)] = groups.get(_group(op), 0.0) + ms / max(n_fw, 1)
    table = m.op_table(a.batch, a.size, a.size)
    attn_ms = groups.get("window attention", 0.0)
    attn_alg = sum(r["flops"] for o, r in zip(m.ops, table) if o.kind == L.OP_WINDOW_ATTN)
    attn_bytes = sum(r["bytes"] for o, r in zip(m.ops, table) if o.kind == L.OP_WINDOW_ATTN)
    attn_exec = attention_executed_flops(m, a.batch, a.size)
    res = {"workload": f"Swin-tiny centered-instance inference forward, {a.batch} crops of {a.size} x {a.size}, 13 nodes, output stride 2, exact fp32",
           "forwards_per_loop": a.forwards, "repeats": a.repeats, "outputs_finite": finite, "parameters": m.num_parameters(),
           "median_ms_per_repeat": [round(x, 3) for x in medians], "median_ms": round(statistics.median(medians), 3), "spread_ms": round(max(medians) - min(medians), 3),
           "per_op_ms": {k: round(v, 3) for k, v in sorted(groups.items(), key=lambda kv: -kv[1])},
           "window_attention": {"ms": round(attn_ms, 3), "algorithmic_gflop": round(attn_alg / 1e9, 2), "executed_gflop": round(attn_exec / 1e9, 2),
                                "executed_tflops": round(attn_exec / (attn_ms * 1e-3) / 1e12, 2) if attn_ms > 0 else None,
                                "share_of_fp32_matrix_peak": round(attn_exec / (attn_ms * 1e-3) / 1e12 / MFMA_F32_PEAK_TFLOPS, 4) if attn_ms > 0 else None,
                                "algorithmic_gbytes": round(attn_bytes / 1e9, 3),
                                "share_of_8_tbps": round(attn_bytes / (attn_ms * 1e-3) / 1e12 / HBM_TBPS, 4) if attn_ms > 0 else None},
           "context_only": "ConvNeXt-tiny's exact forward at the same shape is 87-88 ms (README); a different network, not a baseline"}
    print("| op group | ms |\n|---|---|")
    for k, v in res["per_op_ms"].items():
        print(f"| {k} | {v:.2f} |")
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
