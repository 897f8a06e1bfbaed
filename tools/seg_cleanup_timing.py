"""Timing of the mask cleanup of the bottom-up grouping (``ph_seg_cleanup``, csrc/seg_cleanup_kernels.hip) on the maps of ``tools/seg_timing.py``:
8 frames of 256 x 256 head maps, ``--instances`` synthetic instances per frame; ``--speckle F`` turns that fraction of the foreground pixels off, so that
the instances have pin-holes and loose fragments to clean.  Reported (warmed, median):

* the eight cleanup launches of one batch on the device (device events), beside the grouping launches they follow;
* the stage end to end with cleanup on the device: launches + the one host read + per-instance masks with their holes;
* the same stage with the cleanup on the host instead: the device grouping, then ``clean_label_map`` per frame;
* where SciPy is importable, the reference's routine (``label`` + ``binary_fill_holes`` per instance) on the device grouping's label map.

    python tools/seg_cleanup_timing.py [--frames 8] [--size 256] [--instances 12] [--gate] [--speckle 0.03] [--iters 30]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--instances", type=int, default=12)
    ap.add_argument("--gate", action="store_true")
    ap.add_argument("--speckle", type=float, default=0.03)
    ap.add_argument("--iters", type=int, default=30)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("seg_cleanup_timing needs the GPU")
    dev = "cuda:0"
    B, h, stride = args.frames, args.size, 2
    fg_h, hm_h, off_h = synthetic_maps(B, args.instances, h, stride, 7)
    if args.speckle > 0:
        drop = torch.from_numpy(np.random.default_rng(11).random(tuple(fg_h.shape)) < args.speckle)
        fg_h[drop & (fg_h > 0.5)] = 0.05
    fg, hm, off = fg_h.to(dev), hm_h.to(dev), off_h.to(dev)
    alpha = 2.0 if args.gate else None
    kw = dict(fg_threshold=0.5, peak_threshold=0.2, output_stride=stride, max_instances=None, center_nms_kernel=3, distance_gate_alpha=alpha, distance_gate_iters=3)

    # the cleanup launches alone, on the label map the device grouping leaves
    hd = S.group_enqueue(fg, hm, off, 0.5, 0.2, stride, None, 3, alpha, 3)
    small, labels = hd["dev"][0], hd["dev"][1]
    plain = S.group_finish(hd)
    lib, P, st = L.lib(), (lambda t: C.c_void_p(t.data_ptr())), L.current_stream_ptr()
    mc, hole_cap = S.DEFAULT_MAX_CENTERS, S.DEFAULT_HOLE_CAP
    pool = 2 * (h + 2) * ((h + 2 + 63) // 64)
    rec = torch.empty(2 * B * mc + 2 * B, dtype=torch.int32, device=dev)
    holes = torch.empty((B, hole_cap, 2), dtype=torch.int32, device=dev)
    need = int(lib.ph_seg_cleanup_scratch_bytes(B, h, h, mc, pool))
    scratch = torch.empty((need + 7) // 8, dtype=torch.int64, device=dev)
    cleaned = torch.empty_like(labels)

    def cleanup():
        L.check(lib.ph_seg_cleanup(P(labels), B, h, h, P(small[: 2 * B]), mc, labels.element_size(), P(cleaned), P(rec), P(holes), hole_cap, pool, P(scratch), need, st))

    for _ in range(3):
        cleanup()
    torch.cuda.synchronize()
    r = rec.cpu().numpy()
    print(f"{B} frames of {h} x {h} maps: centres per frame {[len(c) for c in plain.centers]}, foreground {float((fg > 0.5).float().mean()):.2f}, speckle {args.speckle}; "
          f"holes filled per frame {r[2 * B * mc : 2 * B * mc + B].tolist()}, pixels of dropped fragments {int((labels != cleaned).sum())}")
    print(f"ph_seg_cleanup (8 launches): {median_event_us(cleanup, args.iters):.1f} us per batch")

    def device_stage():
        g = S.group_instances_from_offsets(fg, hm, off, mask_cleanup=True, **kw)
        return [g.instances(b, stride) for b in range(B)]

    def plain_stage():
        g = S.group_instances_from_offsets(fg, hm, off, **kw)
        return [g.instances(b, stride) for b in range(B)]

    def host_cleanup_stage():
        g = S.group_instances_from_offsets(fg, hm, off, **kw)
        g.holes = []
        for b in range(B):
            g.labels[b], hol, g.counts[b] = S.clean_label_map(g.labels[b], len(g.centers[b]))
            g.holes.append(hol)
        return [g.instances(b, stride) for b in range(B)]

    d_inst, h_inst = device_stage(), host_cleanup_stage()
    same = all(len(a) == len(b) and all(np.array_equal(x["mask"], y["mask"]) for x, y in zip(a, b)) for a, b in zip(d_inst, h_inst))
    t_p = median_wall_us(plain_stage, max(5, args.iters // 3))
    t_d = median_wall_us(device_stage, max(5, args.iters // 3))
    t_h = median_wall_us(host_cleanup_stage, max(3, args.iters // 10))
    print(f"stage end to end without cleanup: {t_p:.0f} us per batch; with cleanup on the device: {t_d:.0f} us")
    print(f"device grouping + host clean_label_map: {t_h:.0f} us per batch ({t_h / t_d:.1f} x the device stage); results identical: {same}")
    try:
        from scipy.ndimage import binary_fill_holes, label
    except ImportError:
        print("SciPy is not importable: the reference's routine was not timed")
        return

    def scipy_stage():
        g = S.group_instances_from_offsets(fg, hm, off, **kw)
        out = []
        for b in range(B):
            frame = []
            for k in np.nonzero(g.counts[b] > 0)[0]:
                m = g.labels[b] == k
                cc, n = label(m)
                if n > 1:
                    c = np.bincount(cc.ravel())
                    c[0] = 0
                    m = cc == int(c.argmax())
                frame.append(binary_fill_holes(m))
            out.append(frame)
        return out

    s_inst = scipy_stage()
    same = all(len(a) == len(b) and all(np.array_equal(x["mask"], y) for x, y in zip(a, b)) for a, b in zip(d_inst, s_inst))
    t_s = median_wall_us(scipy_stage, max(3, args.iters // 10))
    print(f"device grouping + the reference's SciPy routine per instance: {t_s:.0f} us per batch ({t_s / t_d:.1f} x the device stage); results identical: {same}")


if __name__ == "__main__":
    main()
