"""Time the training step of a ``bottomup_segmentation`` UNet and the rendering of its targets on one MI355X.

    python tools/seg_train_timing.py [--batch 8] [--size 512] [--filters 32] [--instances 6] [--steps 20] [--warmup 5]

Prints one JSON line: milliseconds per ``training_step`` (HIP events around ``steps`` steps after ``warmup``), and per call of
``SegmentationTargetGenerator`` on device masks against the same generator's torch form on the same device tensors.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--filters", type=int, default=32)
    ap.add_argument("--instances", type=int, default=6)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()

    from sleap_nn_amd.architectures.model import Model
    from sleap_nn_amd.data import segmentation_maps as SM
    from sleap_nn_amd.training.segmentation import SegmentationTrainingModule

    dev = torch.device("cuda", 0)
    bb = {"in_channels": 1, "kernel_size": 3, "filters": a.filters, "filters_rate": 2, "max_stride": 16, "stem_stride": None, "middle_block": True,
          "up_interpolate": True, "stacks": 1, "convs_per_block": 2, "output_stride": 2}
    heads = {"segmentation": {"output_stride": 2, "loss_weight": 1.0}, "center": {"sigma": 4.0, "output_stride": 2, "loss_weight": 1.0},
             "offsets": {"output_stride": 2, "loss_weight": 0.1}}
    m = Model("unet", bb, heads, "bottomup_segmentation").init_xavier_(seed=1)
    tm = SegmentationTrainingModule(m, dev, lr=1e-4)
    g = torch.Generator().manual_seed(2)
    B, S, I = a.batch, a.size, a.instances
    img = torch.randint(0, 256, (B, 1, S, S), dtype=torch.uint8, generator=g).to(dev)
    yy, xx = torch.meshgrid(torch.arange(S), torch.arange(S), indexing="ij")
    masks = torch.zeros((B, I, S, S), dtype=torch.uint8)
    for b in range(B):
        for i in range(I):
            cx, cy, r = (torch.rand(3, generator=g) * torch.tensor([S, S, S / 8.0]) + torch.tensor([0.0, 0.0, S / 16.0])).tolist()
            masks[b, i] = ((xx - cx) ** 2 + (yy - cy) ** 2 <= r * r).to(torch.uint8)
    masks = masks.to(dev)
    n = torch.full((B,), I, dtype=torch.int32, device=dev)
    gen = SM.SegmentationTargetGenerator("bottomup_segmentation", heads)
    batch = {"image": img, **gen(masks, n)}

    def torch_form():
        cent, area = SM._stats_torch(masks, n)
        SM._foreground_torch(masks, n, 2, False)
        SM._center_torch(masks, n, 2, 4.0, cent)
        SM._offsets_torch(masks, n, 2, cent, area)

    res = {"batch": B, "size": S, "filters": a.filters, "instances": I,
           "train_step_ms": timed(lambda: tm.training_step(batch), a.steps, a.warmup),
           "targets_kernel_ms": timed(lambda: gen(masks, n), a.steps, a.warmup),
           "targets_torch_on_device_ms": timed(torch_form, a.steps, a.warmup)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
