"""The Swin-tiny training step at cfg4's shape (centered-instance, 64 crops of 384 x 384, 13 nodes, output stride 2), and its backward by op group.

    python tools/swint_train_timing.py [--batch 64] [--size 384] [--steps 10] [--repeats 3] [--out profiles/swint_train_timing.json]

The network step is forward + MSE + backward + Adam (TrainingModule.training_step, stochastic depth on at the reference's 0.1: the scale passes are part of
the step); the backward alone is ph_model_backward between its own first and last HIP event
(profiling on).  Each timed loop is `--steps` steps behind untimed warm-up steps (at least
three, and at least benchlegs.common.WARM_MS of wall time), every step between two device events; `--repeats` loops.  Reported: the median of every repeat and
the spread between those medians (max - min).  A last, untimed pass takes the backward's per-op split from ph_model_backward_profile_read (HIP events around
every op's step of the reverse sweep, one more between a Linear's weight-gradient and data-gradient GEMMs), grouped into window-attention backward,
weight-gradient GEMMs, data-gradient GEMMs, LayerNorm backward, patch-merge backward and tail (losses, heads, decoder, middle, stem).  For the attention
backward alone: the FLOPs it executes (full 32-token MFMA tiles, dead rows and columns included) against the fp32 matrix peak, and its algorithmic bytes (qkv
and the output gradient read once, the qkv gradient written once) against 8 TB/s.  If the training workspaces of `--batch` crops do not fit, the tool falls
back to half the batch and says so.  Needs an MI355X: there is no CPU path.
"""
from __future__ import annotations

import argparse
import ctypes as C
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
from sleap_nn_amd.training.module import TrainingModule  # noqa: E402
from tools.swint_timing import HBM_TBPS, SWINT_BB  # noqa: E402

GROUPS = ("window-attention backward", "weight-gradient GEMMs", "data-gradient GEMMs (+ residual fan-out)", "LayerNorm backward", "patch-merge backward",
          "tail (losses, heads, decoder, middle, stem, GELU)")


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


def attention_bwd_executed_flops(model, batch: int, size: int) -> float:
    """What window_attn_bwd_kernel issues per (window, head), T = ceil(N / 32): pass 1 S^T and dP^T (2 x 16 T^2) + dq^T (16 T^2), pass 2 S and dP (2 x 16 T^2)
    + dV^T and dK^T (2 x 16 T^2) = 112 T^2 v_mfma_f32_32x32x2_f32 of 4096 FLOPs."""
    total = 0.0
    for op, row in zip(model.ops, model.op_table(batch, size, size)):
        if op.kind != L.OP_WINDOW_ATTN:
            continue
        h, w = row["out_hw"]
        ws, t = op.ksize, (op.ksize * op.ksize + 31) // 32
        total += batch * ((h + ws - 1) // ws) * ((w + ws - 1) // ws) * op.cin1 * 112 * t * t * 4096.0
    return total


def _run(batch: int, size: int, steps: int, repeats: int) -> dict:
    dev = torch.device("cuda", 0)
    crops = torch.randint(0, 256, (batch, 1, size, size), dtype=torch.uint8, generator=torch.Generator().manual_seed(4321)).to(dev)
    m = Model("swint", SWINT_BB, CFG4_HEADS, "centered_instance").init_xavier_(seed=1234, head_scale=0.05)
    tm = TrainingModule(m, "cuda:0", lr=1e-4, swint_training=True)
    shape = tuple(tm.model.forward(crops[:1])[m.heads[0].name].shape[1:])
    tgt = torch.rand((batch,) + shape, generator=torch.Generator().manual_seed(7)).to(dev) * 0.5
    batch_d = {"image": crops, m.heads[0].name: tgt}
    step = lambda: tm.training_step(batch_d)  # noqa: E731
    step_med, bwd_med = [], []
    for _ in range(repeats):
        _warm(step)
        step_med.append(statistics.median(_timed(step, steps)))
    loss = step()
    torch.cuda.synchronize()
    finite = bool(torch.isfinite(loss).all()) and bool(torch.isfinite(tm.grads).all())
    # the backward alone and its per-op split: HIP events inside ph_model_backward (profiling on), read after every step
    lib = L.lib()
    m.set_profiling(True)
    n = len(m.ops)
    acc, acc_first, loss_ms, k = [0.0] * n, [0.0] * n, 0.0, steps * repeats
    for _ in range(repeats):
        _warm(step)
        totals = []
        for _ in range(steps):
            step()
            op_ms, first, lm = (C.c_double * n)(), (C.c_double * n)(), C.c_double()
            L.check(lib.ph_model_backward_profile_read(m._handle, op_ms, first, n, C.byref(lm)))
            for i in range(n):
                acc[i] += op_ms[i] / k
                acc_first[i] += first[i] / k
            loss_ms += lm.value / k
            totals.append(lm.value + sum(op_ms))
        bwd_med.append(statistics.median(totals))
    m.set_profiling(False)
    groups = {g: 0.0 for g in GROUPS}
    groups[GROUPS[5]] += loss_ms
    enc_end = max(i for i, o in enumerate(m.ops) if o.label == "backbone.enc.norm")
    for i, op in enumerate(m.ops):
        if op.kind == L.OP_WINDOW_ATTN:
            groups[GROUPS[0]] += acc[i]
        elif op.kind == L.OP_LINEAR and i <= enc_end:
            groups[GROUPS[1]] += acc_first[i]
            groups[GROUPS[2]] += acc[i] - acc_first[i]
        elif op.kind == L.OP_LAYERNORM and i <= enc_end and i > 1:
            groups[GROUPS[3]] += acc[i]
        elif op.kind == L.OP_PATCH_MERGE:
            groups[GROUPS[4]] += acc[i]
        else:
            groups[GROUPS[5]] += acc[i]
    table = m.op_table(batch, size, size)
    attn_ms = groups[GROUPS[0]]
    attn_exec = attention_bwd_executed_flops(m, batch, size)
    # qkv (3C) and the output gradient (C) read, the qkv gradient (3C) written: 7C floats per token
    attn_bytes = sum(4.0 * 7 * o.cout * r["out_hw"][0] * r["out_hw"][1] * batch for o, r in zip(m.ops, table) if o.kind == L.OP_WINDOW_ATTN)
    return {"workload": f"Swin-tiny centered-instance training step, {batch} crops of {size} x {size}, 13 nodes, output stride 2, exact fp32, stochastic depth 0.1",
            "steps_per_loop": steps, "repeats": repeats, "finite": finite, "parameters": m.num_parameters(),
            "step_median_ms_per_repeat": [round(x, 3) for x in step_med], "step_median_ms": round(statistics.median(step_med), 3),
            "step_spread_ms": round(max(step_med) - min(step_med), 3),
            "backward_median_ms_per_repeat": [round(x, 3) for x in bwd_med], "backward_median_ms": round(statistics.median(bwd_med), 3),
            "backward_spread_ms": round(max(bwd_med) - min(bwd_med), 3),
            "backward_per_group_ms": {g: round(v, 3) for g, v in groups.items()},
            "window_attention_backward": {"ms": round(attn_ms, 3), "executed_gflop": round(attn_exec / 1e9, 2),
                                          "executed_tflops": round(attn_exec / (attn_ms * 1e-3) / 1e12, 2) if attn_ms > 0 else None,
                                          "share_of_fp32_matrix_peak": round(attn_exec / (attn_ms * 1e-3) / 1e12 / MFMA_F32_PEAK_TFLOPS, 4) if attn_ms > 0 else None,
                                          "algorithmic_gbytes": round(attn_bytes / 1e9, 3),
                                          "share_of_8_tbps": round(attn_bytes / (attn_ms * 1e-3) / 1e12 / HBM_TBPS, 4) if attn_ms > 0 else None},
            "context_only": "ConvNeXt-tiny's train step at the same shape is 341 ms (README); a different network, not a baseline"}


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--size", type=int, default=384)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    if a.steps < 10 or a.repeats < 3:
        ap.error("at least 10 steps per loop and 3 repeats")
    if not torch.cuda.is_available():
        raise SystemExit("swint_train_timing needs an MI355X (no CPU path)")
    try:
        res = _run(a.batch, a.size, a.steps, a.repeats)
    except torch.OutOfMemoryError:
        torch.cuda.empty_cache()
        res = _run(a.batch // 2, a.size, a.steps, a.repeats)
        res["note"] = f"the training workspaces of {a.batch} crops did not fit: measured at {a.batch // 2}"
    print("| backward op group | ms |\n|---|---|")
    for k, v in res["backward_per_group_ms"].items():
        print(f"| {k} | {v:.2f} |")
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
