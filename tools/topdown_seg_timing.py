"""Timing of the top-down segmentation stage 2 (inference/layers/topdown_segmentation.py, ``ph_seg_place_crops`` in csrc/seg_kernels.hip).

The case: ``--frames`` frames of ``--size`` x ``--size`` with ``--crops`` crops each, crop masks of ``--mask`` x ``--mask`` decoded to ``--extent`` x
``--extent`` image pixels at random origins (some spilling over the frame's edges).  Reported (warmed, median):

* the place launch (device events), with the bytes it stores against the 8 TB/s HBM peak, and a bare ``zero_()`` of the same buffer: the store floor;
* the stage-2 host read: threshold / count / sum of the crop probabilities (``ph_seg_semantic``), the asynchronous copies of the masks and the record
  into pinned memory and the wait for them (wall clock: this is what ``TopDownSegmentationLayer`` waits for per batch after the crop network);
* the host placement of the same crops (NumPy, wall clock), and a check that both placements are identical.

    python tools/topdown_seg_timing.py [--frames 8] [--crops 8] [--size 1024] [--mask 80] [--extent 160] [--iters 20]
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from sleap_nn_amd.inference.ops.segmentation import place_crop_masks, semantic_enqueue, semantic_finish  # noqa: E402

HBM_PEAK = 8.0e12


def median_event_us(fn, iters):
    times = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) * 1e3)
    return statistics.median(times)


def median_wall_us(fn, iters):
    times = []
    for _ in range(iters):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        times.append((time.perf_counter() - t) * 1e6)
    return statistics.median(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--crops", type=int, default=8)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--mask", type=int, default=80)
    ap.add_argument("--extent", type=int, default=160)
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    dev = "cuda:0"
    g = np.random.default_rng(0)
    B, P, S, n = a.frames, a.crops, a.size, a.frames * a.crops
    probs = torch.from_numpy(g.random((n, 1, a.mask, a.mask)).astype(np.float32)).to(dev)
    origins = g.integers(-a.extent // 2, S - a.extent // 2, size=(n, 2))
    extents = np.full((n, 2), a.extent)
    pos = torch.arange(n, dtype=torch.int32, device=dev)
    hd = semantic_enqueue(probs, 0.5, host_masks=True)
    masks_dev = hd["mask_dev"]
    masks_host, _c, _s = semantic_finish(hd)
    geo_o, geo_e = torch.from_numpy(origins).to(dev), torch.from_numpy(extents).to(dev)

    out = place_crop_masks(masks_dev, pos, geo_o, geo_e, (S, S), P)
    want = place_crop_masks(masks_host.astype(np.uint8), np.arange(n), origins, extents, (S, S), P)
    assert np.array_equal(out.cpu().numpy(), want), "device and host placement differ"
    for _ in range(3):
        place_crop_masks(masks_dev, pos, geo_o, geo_e, (S, S), P)
    nbytes = B * P * S * S
    t_place = median_event_us(lambda: place_crop_masks(masks_dev, pos, geo_o, geo_e, (S, S), P), a.iters)
    t_zero = median_event_us(lambda: out.zero_(), a.iters)
    print(f"case: {B} frames x {P} crops, frame {S} x {S}, masks {a.mask} x {a.mask} -> {a.extent} x {a.extent}; output {nbytes / 1e6:.0f} MB")
    print(f"ph_seg_place_crops (with the output's allocation): {t_place:.1f} us -> {nbytes / t_place / 1e3:.0f} GB/s stored = {nbytes / (t_place * 1e-6) / HBM_PEAK:.3f} of 8 TB/s")
    print(f"zero_() of the same buffer (store floor): {t_zero:.1f} us -> {nbytes / t_zero / 1e3:.0f} GB/s")
    t_read = median_wall_us(lambda: semantic_finish(semantic_enqueue(probs, 0.5, host_masks=True)), a.iters)
    print(f"stage-2 host read (ph_seg_semantic on {n} crops, masks + record to pinned memory, wait): {t_read:.1f} us")
    t_host = median_wall_us(lambda: place_crop_masks(masks_host.astype(np.uint8), np.arange(n), origins, extents, (S, S), P), max(1, a.iters // 10))
    print(f"host placement of the same crops (NumPy): {t_host:.1f} us")


if __name__ == "__main__":
    main()
