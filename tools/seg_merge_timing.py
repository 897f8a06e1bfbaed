"""Timing of the fragment merge of the bottom-up grouping (``ph_seg_merge_tables``, csrc/seg_merge_kernels.hip, and the host graph of
``inference/ops/segmentation_merge.py``) on the maps of ``tools/seg_timing.py``: 8 frames of 256 x 256 head maps, ``--instances`` synthetic instances per
frame (overlapping disks abut, so the graph has edges).  Reported (warmed, median):

* the four merge launches of one batch on the device (device events);
* the stage end to end with the merge off and on: launches + the one host read + the host graph + per-instance masks;
* the same stage with the tables computed on the host instead: the device grouping, then ``merge_tables_host`` per frame and the same graph;
* where SciPy is importable, the reference's pairwise routine (two ``binary_dilation`` per pair over the full frame) on the device grouping's label map.

    python tools/seg_merge_timing.py [--frames 8] [--size 256] [--instances 12] [--gate] [--dilate 1] [--iters 30]
"""
import argparse
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402
from seg_timing import median_event_us, median_wall_us, synthetic_maps  # noqa: E402

from sleap_nn_amd import _lib as L  # noqa: E402
from sleap_nn_amd.inference.ops import segmentation as S  # noqa: E402
from sleap_nn_amd.inference.ops import segmentation_merge as M  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--instances", type=int, default=12)
    ap.add_argument("--gate", action="store_true")
    ap.add_argument("--dilate", type=int, default=1)
    ap.add_argument("--iters", type=int, default=30)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("seg_merge_timing needs the GPU")
    dev = "cuda:0"
    B, h, stride = args.frames, args.size, 2
    fg_h, hm_h, off_h = synthetic_maps(B, args.instances, h, stride, 7)
    fg, hm, off = fg_h.to(dev), hm_h.to(dev), off_h.to(dev)
    alpha = 2.0 if args.gate else None
    kw = dict(fg_threshold=0.5, peak_threshold=0.2, output_stride=stride, max_instances=None, center_nms_kernel=3, distance_gate_alpha=alpha, distance_gate_iters=3)
    mkw = S._merge_kw("greedy", (0.85, 0.6, 0.4), 1.0, 0.25, args.dilate, 0.5)

    # the merge launches alone, on the label map the device grouping leaves
    hd = S.group_enqueue(fg, hm, off, 0.5, 0.2, stride, None, 3, alpha, 3)
    small, labels = hd["dev"][0], hd["dev"][1]
    plain = S.group_finish(hd)
    lib, P, st = L.lib(), (lambda t: C.c_void_p(t.data_ptr())), L.current_stream_ptr()
    mc, edge_cap = S.DEFAULT_MAX_CENTERS, M.DEFAULT_EDGE_CAP
    mom = torch.empty((B, mc, 4), dtype=torch.float64, device=dev)
    erec = torch.empty(B + B * edge_cap * 5, dtype=torch.int32, device=dev)
    need = int(lib.ph_seg_merge_scratch_bytes(B, h, h, mc))
    scratch = torch.empty((need + 7) // 8, dtype=torch.int64, device=dev)
    cen = small[2 * B : 2 * B + 2 * B * mc]

    def tables():
        L.check(lib.ph_seg_merge_tables(P(labels), P(hm), P(off), B, h, h, stride, max(1, args.dilate), P(cen), P(small[: 2 * B]), mc, labels.element_size(), P(mom),
                                        P(erec[:B]), P(erec[B:]), edge_cap, P(scratch), need, st))

    for _ in range(3):
        tables()
    torch.cuda.synchronize()
    print(f"{B} frames of {h} x {h} maps: centres per frame {[len(c) for c in plain.centers]}, foreground {float((fg > 0.5).float().mean()):.2f}, dilate {args.dilate}; "
          f"touching pairs per frame {erec[:B].cpu().tolist()}")
    print(f"ph_seg_merge_tables (4 launches): {median_event_us(tables, args.iters):.1f} us per batch")

    def plain_stage():
        g = S.group_instances_from_offsets(fg, hm, off, **kw)
        return [g.instances(b, stride) for b in range(B)]

    def device_stage():
        g = S.group_instances_from_offsets(fg, hm, off, merge_fragments=True, merge_dilate=args.dilate, **kw)
        return [g.instances(b, stride) for b in range(B)]

    def host_tables_stage():
        g = S.group_instances_from_offsets(fg, hm, off, **kw)
        t = []
        for b in range(B):
            _T, mo, ed, ri = M.merge_tables_host(g.labels[b], hm_h[b, 0].numpy(), off_h[b].numpy(), g.centers[b], len(g.centers[b]), stride, args.dilate)
            t.append((ed, ri, mo))
        g = S.merge_grouping(g, t, stride, mkw)
        return [g.instances(b, stride) for b in range(B)]

    p_inst, d_inst, h_inst = plain_stage(), device_stage(), host_tables_stage()
    same = all(len(a) == len(b) and all(np.array_equal(x["mask"], y["mask"]) for x, y in zip(a, b)) for a, b in zip(d_inst, h_inst))
    t_p = median_wall_us(plain_stage, max(5, args.iters // 3))
    t_d = median_wall_us(device_stage, max(5, args.iters // 3))
    t_h = median_wall_us(host_tables_stage, max(3, args.iters // 10))
    print(f"instances per frame without the merge {[len(f) for f in p_inst]}, with it {[len(f) for f in d_inst]}")
    print(f"stage end to end with the merge off: {t_p:.0f} us per batch; on, tables on the device: {t_d:.0f} us")
    print(f"device grouping + host merge_tables_host: {t_h:.0f} us per batch ({t_h / t_d:.1f} x the device stage); results identical: {same}")
    try:
        from scipy.ndimage import binary_dilation
    except ImportError:
        print("SciPy is not importable: the reference's routine was not timed")
        return

    def scipy_contacts():
        g = S.group_instances_from_offsets(fg, hm, off, **kw)
        out = []
        for b in range(B):
            masks = [g.labels[b] == k for k in np.nonzero(g.counts[b] > 0)[0]]
            frame = {}
            for i in range(len(masks)):
                for j in range(i + 1, len(masks)):
                    ov = int((binary_dilation(masks[i], iterations=max(1, args.dilate)) & masks[j]).sum() + (masks[i] & binary_dilation(masks[j], iterations=max(1, args.dilate))).sum())
                    if ov:
                        frame[(i, j)] = ov
            out.append(frame)
        return out

    t_s = median_wall_us(scipy_contacts, max(3, args.iters // 10))
    print(f"device grouping + the reference's pairwise SciPy dilations (contacts only): {t_s:.0f} us per batch ({t_s / t_d:.1f} x the device stage)")


if __name__ == "__main__":
    main()
