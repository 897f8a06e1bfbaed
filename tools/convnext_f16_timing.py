"""The cfg4 inference forward (ConvNeXt-tiny centered-instance, 64 crops of 384 x 384) in the exact and the fp16 precision, in ONE process.

    python tools/convnext_f16_timing.py [--batch 64] [--forwards 20] [--repeats 3] [--out result.json]

Both models hold the same weights.  Each timed loop is `--forwards` forwards, every forward between two device events, behind untimed
warm-up calls (at least three, and at least benchlegs.common.WARM_MS of wall time: a loop must not start at the clocks of an idling GPU);
the loops of the two precisions alternate, `--repeats` times each.  Reported per precision: the median forward of every repeat and the
spread between those medians (max - min); the fp16 forward counts as faster only if the gap between the precisions exceeds that spread.
A last, untimed pass takes the per-op split from ph_model_set_profiling (HIP events around every op), grouped by op kind, and the
distance between the two precisions' heads.  Needs an MI355X: there is no CPU path.
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

from benchlegs.common import CFG4_BB, CFG4_HEADS, WARM_MS  # noqa: E402
from sleap_nn_amd import _lib as L  # noqa: E402
from sleap_nn_amd.architectures.model import Model  # noqa: E402

KIND_NAMES = {L.OP_CONV: "conv3x3 (middle + decoder)", L.OP_LINEAR: "linear (CNBlock MLP)", L.OP_PATCH_CONV: "conv2x2/s2", L.OP_PATCH_STEM: "patch stem", L.OP_DWCONV: "depthwise 7x7 (+LayerNorm)",
              L.OP_LAYERNORM: "layernorm (standalone)", L.OP_UPSAMPLE: "bilinear x2", L.OP_POOL: "pool", L.OP_HEAD: "head"}


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


def _per_op(model, fn, n):
    model.set_profiling(True)
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    op_ms, n_fw = model.read_profile()
    model.set_profiling(False)
    groups = {}
    for op, ms in zip(model.ops, op_ms):
        groups[KIND_NAMES.get(op.kind, str(op.kind))] = groups.get(KIND_NAMES.get(op.kind, str(op.kind)), 0.0) + ms / max(n_fw, 1)
    by_width = {}
    for op, ms in zip(model.ops, op_ms):
        if op.kind == L.OP_LINEAR:
            c = min(op.cin0, op.cout)
            by_width[c] = by_width.get(c, 0.0) + ms / max(n_fw, 1)
    return groups, {f"linear, {c} channels": v for c, v in sorted(by_width.items())}


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
        raise SystemExit("convnext_f16_timing needs an MI355X (no CPU path)")
    dev = torch.device("cuda", 0)
    crops = torch.randint(0, 256, (a.batch, 1, a.size, a.size), dtype=torch.uint8, generator=torch.Generator().manual_seed(4321)).to(dev)
    models = {}
    for prec in ("exact", "fp16"):
        m = Model("convnext", CFG4_BB, CFG4_HEADS, "centered_instance").init_xavier_(seed=1234, head_scale=0.05)
        models[prec] = m.to(dev).set_precision(prec, convnext_f16=True)
    fns = {p: (lambda m=m: m(crops)) for p, m in models.items()}
    medians = {p: [] for p in models}
    for _ in range(a.repeats):
        for p in ("exact", "fp16"):
            _warm(fns[p])
            medians[p].append(statistics.median(_timed(fns[p], a.forwards)))
    heads = {p: {k: v.clone() for k, v in fns[p]().items()} for p in models}
    torch.cuda.synchronize()
    diff = {k: float((heads["fp16"][k] - heads["exact"][k]).abs().max()) / max(1.0, float(heads["exact"][k].abs().max())) for k in heads["exact"]}
    res = {"workload": f"cfg4 inference forward: ConvNeXt-tiny centered-instance, {a.batch} crops of {a.size} x {a.size}, 13 nodes, output stride 2", "forwards_per_loop": a.forwards,
           "repeats": a.repeats, "fp16_vs_exact_head_error": diff}
    for p, m in models.items():
        groups, widths = _per_op(m, fns[p], 5)
        codes = m.last_kernels()
        res[p] = {"median_ms_per_repeat": [round(x, 3) for x in medians[p]], "median_ms": round(statistics.median(medians[p]), 3), "spread_ms": round(max(medians[p]) - min(medians[p]), 3),
                  "per_op_ms": {k: round(v, 3) for k, v in sorted(groups.items(), key=lambda kv: -kv[1])}, "linear_by_width_ms": {k: round(v, 3) for k, v in widths.items()},
                  "kernels": sorted({L.KV_NAMES.get(c, str(c)) for c in codes if c != L.KV_NONE})}
    spread = max(res["exact"]["spread_ms"], res["fp16"]["spread_ms"])
    res["speedup"] = round(res["exact"]["median_ms"] / res["fp16"]["median_ms"], 3)
    res["fp16_faster_by_more_than_spread"] = bool(min(medians["exact"]) - max(medians["fp16"]) > spread)
    print("| op kind | exact ms | fp16 ms |\n|---|---|---|")
    for k in res["exact"]["per_op_ms"]:
        print(f"| {k} | {res['exact']['per_op_ms'][k]:.2f} | {res['fp16']['per_op_ms'].get(k, 0.0):.2f} |")
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
