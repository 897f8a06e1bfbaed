"""The Swin-tiny inference forward at cfg4's shape (centered-instance, 64 crops of 384 x 384) in the exact and the fp16 precision, in ONE process.

    python tools/swint_f16_timing.py [--batch 64] [--size 384] [--forwards 20] [--repeats 3] [--out profiles/swint_f16_timing.json]

Both models hold the same weights; the fp16 one has the handle option swint_f16 set.  Each timed loop is `--forwards` forwards, every forward between
two device events, behind untimed warm-up calls (at least three, and at least benchlegs.common.WARM_MS of wall time); the loops of the two precisions
alternate, `--repeats` times each.  Reported per precision: the median forward of every repeat and the spread between those medians (max - min); the
fp16 forward counts as faster only if the gap between the precisions exceeds that spread.  A last, untimed pass takes the per-op split from
ph_model_set_profiling (HIP events around every op), grouped as tools/swint_timing.py groups it, and the distance between the two precisions' heads.
For the attention kernels alone: the FLOPs they execute (full 32-token MFMA tiles, dead rows and columns included) against the matrix peak of their
operand format, and their algorithmic bytes (qkv read once, output written once, in the storage format) against 8 TB/s.  Needs an MI355X.
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

import swint_timing as S  # noqa: E402
from benchlegs.common import CFG4_HEADS, MFMA_F16_PEAK_TFLOPS, MFMA_F32_PEAK_TFLOPS  # noqa: E402
from sleap_nn_amd import _lib as L  # noqa: E402
from sleap_nn_amd.architectures.model import Model  # noqa: E402


def _per_group(model, fn, n):
    model.set_profiling(True)
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    op_ms, n_fw = model.read_profile()
    model.set_profiling(False)
    groups = {}
    for op, ms in zip(model.ops, op_ms):
        groups[S._group(op)] = groups.get(S._group(op), 0.0) + ms / max(n_fw, 1)
    return groups


def _attention(model, ms, batch, size, bytes_per_value, peak):
    table = model.op_table(batch, size, size)
    executed = S.attention_executed_flops(model, batch, size)  # (the same tile count on either pipe: 16 x 4096 = 2 x 32768 FLOPs per tile pair)
    nbytes = sum(r["bytes"] for o, r in zip(model.ops, table) if o.kind == L.OP_WINDOW_ATTN) * bytes_per_value / 4.0  # (op_table counts 4 bytes per value)
    if ms <= 0:
        return {"ms": 0.0}
    return {"ms": round(ms, 3), "executed_gflop": round(executed / 1e9, 2), "executed_tflops": round(executed / (ms * 1e-3) / 1e12, 2),
            "matrix_peak_tflops": peak, "share_of_matrix_peak": round(executed / (ms * 1e-3) / 1e12 / peak, 4),
            "algorithmic_gbytes": round(nbytes / 1e9, 3), "achieved_gbps": round(nbytes / (ms * 1e-3) / 1e9, 1), "share_of_8_tbps": round(nbytes / (ms * 1e-3) / 1e12 / S.HBM_TBPS, 4)}


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--size", type=int, default=384)
    ap.add_argument("--forwards", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "swint_f16_timing.json"))
    a = ap.parse_args(argv)
    if a.forwards < 20 or a.repeats < 3:
        ap.error("at least 20 forwards per loop and 3 repeats")
    if not torch.cuda.is_available():
        raise SystemExit("swint_f16_timing needs an MI355X (no CPU path)")
    dev = torch.device("cuda", 0)
    crops = torch.randint(0, 256, (a.batch, 1, a.size, a.size), dtype=torch.uint8, generator=torch.Generator().manual_seed(4321)).to(dev)
    models = {}
    for prec in ("exact", "fp16"):
        m = Model("swint", S.SWINT_BB, CFG4_HEADS, "centered_instance").init_xavier_(seed=1234, head_scale=0.05)
        models[prec] = m.to(dev).set_precision(prec, swint_f16=True)
    fns = {p: (lambda m=m: m(crops)) for p, m in models.items()}
    medians = {p: [] for p in models}
    for _ in range(a.repeats):
        for p in ("exact", "fp16"):
            S._warm(fns[p])
            medians[p].append(statistics.median(S._timed(fns[p], a.forwards)))
    heads = {p: {k: v.clone() for k, v in fns[p]().items()} for p in models}
    torch.cuda.synchronize()
    diff = {k: float((heads["fp16"][k] - heads["exact"][k]).abs().max()) / max(1.0, float(heads["exact"][k].abs().max())) for k in heads["exact"]}
    res = {"workload": f"Swin-tiny centered-instance inference forward, {a.batch} crops of {a.size} x {a.size}, 13 nodes, output stride 2", "forwards_per_loop": a.forwards,
           "repeats": a.repeats, "fp16_vs_exact_head_error": diff, "outputs_finite": all(bool(torch.isfinite(v).all()) for h in heads.values() for v in h.values())}
    for p, m in models.items():
        groups = _per_group(m, fns[p], 5)
        codes = m.last_kernels()
        res[p] = {"median_ms_per_repeat": [round(x, 3) for x in medians[p]], "median_ms": round(statistics.median(medians[p]), 3), "spread_ms": round(max(medians[p]) - min(medians[p]), 3),
                  "per_op_ms": {k: round(v, 3) for k, v in sorted(groups.items(), key=lambda kv: -kv[1])},
                  "window_attention": _attention(m, groups.get("window attention", 0.0), a.batch, a.size, 4 if p == "exact" else 2, MFMA_F32_PEAK_TFLOPS if p == "exact" else MFMA_F16_PEAK_TFLOPS),
                  "kernels": sorted({L.KV_NAMES.get(c, str(c)) for c in codes if c != L.KV_NONE})}
    spread = max(res["exact"]["spread_ms"], res["fp16"]["spread_ms"])
    res["gap_ms"] = round(res["exact"]["median_ms"] - res["fp16"]["median_ms"], 3)
    res["spread_ms"] = spread
    res["speedup"] = round(res["exact"]["median_ms"] / res["fp16"]["median_ms"], 3)
    res["fp16_faster_by_more_than_spread"] = bool(min(medians["exact"]) - max(medians["fp16"]) > spread)
    res["groups_not_faster_in_fp16"] = [k for k, v in res["exact"]["per_op_ms"].items() if res["fp16"]["per_op_ms"].get(k, 0.0) >= v]
    print("| op group | exact ms | fp16 ms | ratio |\n|---|---|---|---|")
    for k, v in res["exact"]["per_op_ms"].items():
        f = res["fp16"]["per_op_ms"].get(k, 0.0)
        print(f"| {k} | {v:.2f} | {f:.2f} | {v / f if f > 0 else float('nan'):.2f} |")
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
