"""The ConvNeXtV2-nano (``pretrained`` backbone) inference forward at cfg4's shape (centered-instance, 64 crops of 384 x 384, exact fp32), split by op group.

    python tools/convnextv2_timing.py [--batch 64] [--size 384] [--forwards 20] [--repeats 3] [--out profiles/convnextv2_timing.json]

Each timed loop is `--forwards` forwards, every forward between two device events, behind untimed warm-up calls (at least three, and at least
benchlegs.common.WARM_MS of wall time); `--repeats` loops per leg, the legs alternating: the forward with the two-launch GRN (handle option grn_fuse 0), the same
model on the fused GRN plan (grn_fuse 1), ConvNeXt-tiny.  Reported: the median forward of every repeat and the spread between those medians (max - min); the
fused plan counts as faster only if the difference of the medians exceeds both spreads.  Untimed passes then take the per-op split of either plan from
ph_model_set_profiling (HIP events around every op), grouped into stem, depthwise 7x7 + LayerNorm, Linear 1 (+ GELU), GRN, Linear 2 (+ residual), downsampling,
stage norms, decoder, head (fused plan: Linear 1 carries the sums of squares, GRN is the finalize launch, Linear 2 the weight scaling and one GEMM per sample).
For the two-launch GRN alone: its algorithmic bytes (the hidden tensor read twice -- reduction and apply pass -- and written once) against 8 TB/s; the kernels
are bandwidth-bound, so that is their share of peak.  The ConvNeXt-tiny exact forward is re-measured in the same process as context (another network, not a baseline).  Needs an MI355X: there is no CPU path.
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

NANO_BB = {"source": "hf", "model_name": "facebook/convnextv2-nano-22k-224", "in_channels": 3, "output_stride": 2, "max_stride": 32, "mode": "decoder", "normalize": True,
           "filters_rate": 2.0, "convs_per_block": 2, "kernel_size": 3, "up_interpolate": True}
HBM_TBPS = 8.0


def _group(op) -> str:
    if op.kind == L.OP_PATCH_STEM or op.label.endswith("embeddings.layernorm"):
        return "stem (patch conv + LayerNorm)"
    if op.kind == L.OP_GRN:
        return "GRN (reduction + apply)"
    if op.kind == L.OP_DWCONV or op.label.endswith(".layernorm"):
        return "depthwise 7x7 + LayerNorm"
    if op.kind == L.OP_LINEAR:
        return "Linear 2 (+ residual)" if op.flags & L.FLAG_RESIDUAL else "Linear 1 (+ GELU)"
    if op.kind == L.OP_PATCH_CONV or ".downsampling_layer." in op.label:
        return "downsampling (LayerNorm + 2x2/s2 conv)"
    if "hidden_states_norms" in op.label:
        return "stage norms"
    if op.kind == L.OP_HEAD:
        return "head"
    return "decoder (bilinear x2, conv3x3)"


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


def _summary(medians):
    return {"median_ms_per_repeat": [round(x, 3) for x in medians], "median_ms": round(statistics.median(medians), 3), "spread_ms": round(max(medians) - min(medians), 3)}


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--size", type=int, default=384)
    ap.add_argument("--forwards", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "convnextv2_timing.json"))
    a = ap.parse_args(argv)
    if a.forwards < 20 or a.repeats < 3:
        ap.error("at least 20 forwards per loop and 3 repeats")
    if not torch.cuda.is_available():
        raise SystemExit("convnextv2_timing needs an MI355X (no CPU path)")
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(4321)
    rgb = torch.randint(0, 256, (a.batch, 3, a.size, a.size), dtype=torch.uint8, generator=g).to(dev)
    gray = rgb[:, :1].contiguous()
    v2 = Model("pretrained", NANO_BB, CFG4_HEADS, "centered_instance").init_xavier_(seed=1234, head_scale=0.05).to(dev)
    tiny = Model("convnext", CFG4_BB, CFG4_HEADS, "centered_instance").init_xavier_(seed=1234, head_scale=0.05).to(dev)
    f_v2 = lambda: v2(rgb)  # noqa: E731
    f_tiny = lambda: tiny(gray)  # noqa: E731
    med = {"v2": [], "v2_fused": [], "tiny": []}
    for _ in range(a.repeats):  # the legs alternate, so that a drift of the machine lands on all of them
        for key, fn, fuse in (("v2", f_v2, 0), ("v2_fused", f_v2, 1), ("tiny", f_tiny, None)):
            if fuse is not None:
                v2.set_option("grn_fuse", fuse)
            _warm(fn)
            med[key].append(statistics.median(_timed(fn, a.forwards)))

    def split(fuse):
        v2.set_option("grn_fuse", fuse)
        res = f_v2()
        torch.cuda.synchronize()
        v2.set_profiling(True)
        for _ in range(5):
            f_v2()
        torch.cuda.synchronize()
        op_ms, n_fw = v2.read_profile()
        v2.set_profiling(False)
        gr = {}
        for op, ms in zip(v2.ops, op_ms):
            gr[_group(op)] = gr.get(_group(op), 0.0) + ms / max(n_fw, 1)
        return res, gr

    out_f, groups_f = split(1)
    out, groups = split(0)
    finite = all(bool(torch.isfinite(v).all()) for v in out.values())
    plans_differ = max(float((out[k] - out_f[k]).abs().max() / max(1.0, float(out[k].abs().max()))) for k in out)
    d_ms = statistics.median(med["v2"]) - statistics.median(med["v2_fused"])
    spread = max(max(med["v2"]) - min(med["v2"]), max(med["v2_fused"]) - min(med["v2_fused"]))
    table = v2.op_table(a.batch, a.size, a.size)
    grn_ms = groups.get("GRN (reduction + apply)", 0.0)
    hidden_bytes = sum(4.0 * r["cout"] * r["out_hw"][0] * r["out_hw"][1] * a.batch for o, r in zip(v2.ops, table) if o.kind == L.OP_GRN)
    grn_bytes = 3.0 * hidden_bytes
    res = {"workload": f"ConvNeXtV2-nano (pretrained backbone) centered-instance inference forward, {a.batch} crops of {a.size} x {a.size}, 13 nodes, output stride 2, exact fp32",
           "forwards_per_loop": a.forwards, "repeats": a.repeats, "outputs_finite": finite, "parameters": v2.num_parameters(),
           "grn_plan": "grn_fuse 0: grn_reduce_kernel + grn_apply_kernel between the two row GEMMs of a block",
           **_summary(med["v2"]),
           "per_op_ms": {k: round(v, 3) for k, v in sorted(groups.items(), key=lambda kv: -kv[1])},
           "fused_plan": {"grn_plan": "grn_fuse 1: sums of squares from the first GEMM's epilogue, grn_finalize_kernel, per-sample scaled weights and one GEMM per sample",
                          **_summary(med["v2_fused"]), "per_op_ms": {k: round(v, 3) for k, v in sorted(groups_f.items(), key=lambda kv: -kv[1])},
                          "max_difference_from_unfused_outputs_of_scale": plans_differ},
           "unfused_minus_fused_ms": round(d_ms, 3), "larger_spread_ms": round(spread, 3),
           "fused_is_faster_beyond_the_spread": bool(d_ms > spread),
           "grn": {"ms": round(grn_ms, 3), "hidden_tensor_gbytes_all_blocks": round(hidden_bytes / 1e9, 3), "algorithmic_gbytes": round(grn_bytes / 1e9, 3),
                   "tbytes_per_s": round(grn_bytes / (grn_ms * 1e-3) / 1e12, 3) if grn_ms > 0 else None,
                   "share_of_8_tbps": round(grn_bytes / (grn_ms * 1e-3) / 1e12 / HBM_TBPS, 4) if grn_ms > 0 else None},
           "convnext_tiny_same_process": {"workload": "ConvNeXt-tiny exact forward at the same shape, 1-channel crops (README: 87-88 ms); context only, another network, not a baseline",
                                          **_summary(med["tiny"])}}
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
