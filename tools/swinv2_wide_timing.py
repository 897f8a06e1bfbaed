"""The Swinv2-tiny window16-256 (``pretrained`` backbone, microsoft/swinv2-tiny-patch4-window16-256 from the table of sizes, behind ``allow_swinv2_wide``) inference forward
at cfg4's shape (centered-instance, 64 crops of 384 x 384, exact fp32), split by op group: the first measurement of the key-tiled cosine window attention kernel
(window_attn_v2_wide_kernel) inside a network.

    python tools/swinv2_wide_timing.py [--batch 64] [--size 384] [--forwards 20] [--repeats 3] [--out profiles/swinv2_wide_timing.json]

The method is tools/swinv2_timing.py's: each timed loop is `--forwards` forwards, every forward between two device events, behind untimed warm-up calls; `--repeats`
loops per leg, the legs alternating (window16-256, window8-256); reported are the median forward of every repeat and the spread between those medians.  Untimed passes
then take the per-op split from ph_model_set_profiling (HIP events around every op).  For the attention launches: milliseconds, the FLOPs they execute (full 32-token MFMA
tiles: per window and head T x T tile pairs of 16 + 16 v_mfma_f32_32x32x2_f32, T = ceil(N / 32)) against the fp32 matrix peak, and their algorithmic bytes (qkv read
once, output written once) against 8 TB/s -- split into the launches of the key-tiled kernel (stages 1 to 3 at 384 x 384: window 16) and of the one-wave kernel (stage 4:
window 8).  The backbone did not run before: there is no earlier time and no speed bar; the window8-256 forward of the same process is context only (another window, the
one-wave kernel throughout).  Needs an MI355X: there is no CPU path.
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
from swinv2_timing import ATT, SWINV2_BB, _group  # noqa: E402

WIDE_BB = dict(NANO_BB, model_name="microsoft/swinv2-tiny-patch4-window16-256", allow_swinv2=True, allow_swinv2_wide=True)


def attention_launches(model, batch: int, size: int, op_ms, n_fw: int) -> dict:
    """Per kernel (key-tiled: window > 8; one-wave: window <= 8): launches, ms, executed FLOPs and algorithmic bytes of the attention ops of one forward."""
    out = {}
    for op, t, row in zip(model.ops, op_ms, model.op_table(batch, size, size)):
        if op.kind != L.OP_WINDOW_ATTN_V2:
            continue
        h, w = row["out_hw"]
        ws, tiles = op.ksize, (op.ksize * op.ksize + 31) // 32
        d = out.setdefault("window_attn_v2_wide_kernel" if ws > 8 else "window_attn_v2_kernel", {"launches": 0, "windows": set(), "ms": 0.0, "flop": 0.0, "bytes": 0.0})
        d["launches"] += 1
        d["windows"].add(ws)
        d["ms"] += t / max(n_fw, 1)
        d["flop"] += batch * ((h + ws - 1) // ws) * ((w + ws - 1) // ws) * op.cin1 * 32 * tiles * tiles * 4096.0
        d["bytes"] += row["bytes"]
    res = {}
    for k, d in out.items():
        s = d["ms"] * 1e-3
        res[k] = {"launches": d["launches"], "window_sides": sorted(d["windows"]), "ms": round(d["ms"], 3), "executed_gflop": round(d["flop"] / 1e9, 2),
                  "executed_tflops": round(d["flop"] / s / 1e12, 2) if s > 0 else None,
                  "share_of_fp32_matrix_peak": round(d["flop"] / s / 1e12 / MFMA_F32_PEAK_TFLOPS, 4) if s > 0 else None,
                  "algorithmic_gbytes": round(d["bytes"] / 1e9, 3), "share_of_8_tbps": round(d["bytes"] / s / 1e12 / HBM_TBPS, 4) if s > 0 else None}
    return res


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--size", type=int, default=384)
    ap.add_argument("--forwards", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "swinv2_wide_timing.json"))
    a = ap.parse_args(argv)
    if a.forwards < 20 or a.repeats < 3:
        ap.error("at least 20 forwards per loop and 3 repeats")
    if not torch.cuda.is_available():
        raise SystemExit("swinv2_wide_timing needs an MI355X (no CPU path)")
    dev = torch.device("cuda", 0)
    rgb = torch.randint(0, 256, (a.batch, 3, a.size, a.size), dtype=torch.uint8, generator=torch.Generator().manual_seed(4321)).to(dev)
    wide = Model("pretrained", WIDE_BB, CFG4_HEADS, "centered_instance").init_xavier_(seed=1234, head_scale=0.05).to(dev)
    w8 = Model("pretrained", SWINV2_BB, CFG4_HEADS, "centered_instance").init_xavier_(seed=1234, head_scale=0.05).to(dev)
    f_wide = lambda: wide(rgb)  # noqa: E731
    f_w8 = lambda: w8(rgb)  # noqa: E731
    med = {"wide": [], "w8": []}
    for _ in range(a.repeats):  # the legs alternate, so that a drift of the machine lands on both
        for key, fn in (("wide", f_wide), ("w8", f_w8)):
            _warm(fn)
            med[key].append(statistics.median(_timed(fn, a.forwards)))
    split = {}
    for key, m, fn in (("wide", wide, f_wide), ("w8", w8, f_w8)):
        out = fn()
        torch.cuda.synchronize()
        m.set_profiling(True)
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
        op_ms, n_fw = m.read_profile()
        m.set_profiling(False)
        ms = {}
        for op, t in zip(m.ops, op_ms):
            ms[_group(op)] = ms.get(_group(op), 0.0) + t / max(n_fw, 1)
        split[key] = {"finite": all(bool(torch.isfinite(v).all()) for v in out.values()), "ms": ms, "attention": attention_launches(m, a.batch, a.size, op_ms, n_fw)}
    table = wide.op_table(a.batch, a.size, a.size)
    ms = split["wide"]["ms"]
    res = {"workload": f"Swinv2-tiny window16-256 (pretrained backbone, HuggingFace Swinv2Backbone, window 16, image_size 256; effective windows 16 / 16 / 16 / 8) centered-instance "
                       f"inference forward, {a.batch} crops of {a.size} x {a.size}, 13 nodes, output stride 2, exact fp32",
           "backbone_config": WIDE_BB, "forwards_per_loop": a.forwards, "repeats": a.repeats, "outputs_finite": split["wide"]["finite"],
           "parameters": wide.num_parameters(), "direct_tflop_per_forward": round(sum(r["flops"] for r in table) / 1e12, 3), "workspace_gbytes": round(wide._workspace.numel() / 1e9, 2),
           **_summary(med["wide"]),
           "per_op_ms": {k: round(v, 3) for k, v in sorted(ms.items(), key=lambda kv: -kv[1])},
           "share_of_forward": {k: round(v / sum(ms.values()), 4) for k, v in sorted(ms.items(), key=lambda kv: -kv[1])},
           "fp32_mfma_peak_tflops": MFMA_F32_PEAK_TFLOPS,
           "cosine_window_attention": split["wide"]["attention"],
           "earlier_time": "none: these windows did not run before; there is no speed bar",
           "window8_256_same_process": {"workload": "Swinv2-tiny window8-256 at the same shape (the one-wave kernel throughout); context only, another window size, not a baseline",
                                        **_summary(med["w8"]), "attention_ms": round(split["w8"]["ms"].get(ATT, 0.0), 3), "cosine_window_attention": split["w8"]["attention"]},
           "not_measured": "not measured: kernel times from a profiler trace, any other batch or frame size, the small / base / large sizes, window12-192, the 12to16 and 12to24 "
                           "checkpoints (window 24), LDS staging of K and V against the register prefetch"}
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
