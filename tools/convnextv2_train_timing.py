"""The ConvNeXtV2-nano (`pretrained` backbone) training step at cfg4's shape (centered-instance, 64 crops of 384 x 384, 13 nodes, output stride 2, exact fp32),
its backward by op kind, the GRN backward against the memory roof, and the same step with the encoder frozen.

    python tools/convnextv2_train_timing.py [--batch 64] [--size 384] [--steps 10] [--repeats 3] [--out profiles/convnextv2_train_timing.json]

The network step is forward + MSE + backward + Adam (TrainingModule.training_step); the backward alone is ph_model_backward between its own first and last HIP
event (profiling on).  Loops, warm-up and the reported medians and spreads are those of tools/swint_train_timing.py: `--steps` steps per loop behind untimed
warm-up steps, every step between two device events, `--repeats` loops, the median of every loop and the spread between those medians.  The per-op split comes
from ph_model_backward_profile_read (HIP events around every op's step of the reverse sweep, one more between a Linear's weight- and data-gradient GEMMs).
GRN backward: the bytes its kernels must move -- the reduction reads x and g, the apply pass reads x and g and writes dx: five passes over the hidden tensor,
against the forward's three -- over its time, as a share of 8 TB/s.  There is no earlier time to compare with: before this tool the backbone did not train.
Needs an MI355X: there is no CPU path.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from benchlegs.common import CFG4_HEADS  # noqa: E402
from sleap_nn_amd import _lib as L  # noqa: E402
from sleap_nn_amd.architectures.model import Model  # noqa: E402
from sleap_nn_amd.training.module import TrainingModule  # noqa: E402
from tools.swint_timing import HBM_TBPS  # noqa: E402
from tools.swint_train_timing import _timed, _warm  # noqa: E402

CNX2_BB = {"source": "hf", "model_name": "facebook/convnextv2-nano-22k-224", "in_channels": 3, "output_stride": 2, "mode": "decoder", "normalize": True, "filters_rate": 2.0,
           "convs_per_block": 2, "kernel_size": 3, "up_interpolate": True}
GROUPS = ("GRN backward", "GELU backward", "weight-gradient GEMMs", "data-gradient GEMMs (+ residual fan-out)", "LayerNorm backward", "depthwise 7x7 backward",
          "patch stem", "tail (losses, heads, decoder)")


def _module(freeze: bool):
    m = Model("pretrained", CNX2_BB, CFG4_HEADS, "centered_instance").init_xavier_(seed=1234, head_scale=0.05)
    return m, TrainingModule(m, "cuda:0", lr=1e-4, pretrained_training=True, freeze_encoder=freeze)


def _loops(m, tm, batch_d, steps: int, repeats: int):
    """-> (step medians per loop, backward medians per loop, per-op ms, per-op ms up to the mid event, loss ms, finite)."""
    step = lambda: tm.training_step(batch_d)  # noqa: E731
    step_med, bwd_med = [], []
    for _ in range(repeats):
        _warm(step)
        step_med.append(statistics.median(_timed(step, steps)))
    loss = step()
    torch.cuda.synchronize()
    finite = bool(torch.isfinite(loss).all()) and bool(torch.isfinite(tm.grads).all())
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
    return step_med, bwd_med, acc, acc_first, loss_ms, finite


def _summary(step_med, bwd_med):
    return {"step_median_ms_per_repeat": [round(x, 3) for x in step_med], "step_median_ms": round(statistics.median(step_med), 3),
            "step_spread_ms": round(max(step_med) - min(step_med), 3),
            "backward_median_ms_per_repeat": [round(x, 3) for x in bwd_med], "backward_median_ms": round(statistics.median(bwd_med), 3),
            "backward_spread_ms": round(max(bwd_med) - min(bwd_med), 3)}


def _run(batch: int, size: int, steps: int, repeats: int) -> dict:
    dev = torch.device("cuda", 0)
    crops = torch.randint(0, 256, (batch, 3, size, size), dtype=torch.uint8, generator=torch.Generator().manual_seed(4321)).to(dev)
    m, tm = _module(False)
    name = m.heads[0].name
    shape = tuple(tm.model.forward(crops[:1])[name].shape[1:])
    tgt = torch.rand((batch,) + shape, generator=torch.Generator().manual_seed(7)).to(dev) * 0.5
    batch_d = {"image": crops, name: tgt}
    step_med, bwd_med, acc, acc_first, loss_ms, finite = _loops(m, tm, batch_d, steps, repeats)
    n_enc = m.backbone.encoder_ops()
    groups = {g: 0.0 for g in GROUPS}
    groups[GROUPS[7]] += loss_ms
    for i, op in enumerate(m.ops):
        if i >= n_enc:
            groups[GROUPS[7]] += acc[i]
        elif op.kind == L.OP_GRN:
            groups[GROUPS[0]] += acc[i]
        elif op.kind == L.OP_GELU:
            groups[GROUPS[1]] += acc[i]
        elif op.kind in (L.OP_LINEAR, L.OP_PATCH_CONV):
            groups[GROUPS[2]] += acc_first[i]
            groups[GROUPS[3]] += acc[i] - acc_first[i]
        elif op.kind == L.OP_LAYERNORM:
            groups[GROUPS[4]] += acc[i]
        elif op.kind == L.OP_DWCONV:
            groups[GROUPS[5]] += acc[i]
        else:
            groups[GROUPS[6]] += acc[i]
    table = m.op_table(batch, size, size)
    grn_ms = groups[GROUPS[0]]
    hidden_bytes = sum(4.0 * o.cout * r["out_hw"][0] * r["out_hw"][1] * batch for o, r in zip(m.ops, table) if o.kind == L.OP_GRN)  # one pass over every block's hidden tensor
    res = {"workload": f"ConvNeXtV2-nano centered-instance training step, {batch} crops of {size} x {size} x 3, 13 nodes, output stride 2, exact fp32, Adam",
           "steps_per_loop": steps, "repeats": repeats, "finite": finite, "parameters": m.num_parameters(), **_summary(step_med, bwd_med),
           "backward_per_group_ms": {g: round(v, 3) for g, v in groups.items()},
           "grn_backward": {"ms": round(grn_ms, 3), "blocks": sum(1 for o in m.ops if o.kind == L.OP_GRN), "hidden_tensor_gbytes": round(hidden_bytes / 1e9, 3),
                            "passes": 5, "algorithmic_gbytes": round(5 * hidden_bytes / 1e9, 3),
                            "share_of_8_tbps": round(5 * hidden_bytes / (grn_ms * 1e-3) / 1e12 / HBM_TBPS, 4) if grn_ms > 0 else None}}
    tm.close()
    del tm, m
    torch.cuda.empty_cache()
    m, tm = _module(True)
    f_step, f_bwd, f_acc, _first, _loss_ms, f_finite = _loops(m, tm, batch_d, steps, repeats)
    res["frozen_encoder"] = {**_summary(f_step, f_bwd), "finite": f_finite, "encoder_ops": n_enc, "encoder_backward_ms": round(sum(f_acc[:n_enc]), 3),
                             "trainable_parameters": sum(hi - lo for lo, hi in tm._ranges)}
    tm.close()
    return res


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
        raise SystemExit("convnextv2_train_timing needs an MI355X (no CPU path)")
    res = _run(a.batch, a.size, a.steps, a.repeats)
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
