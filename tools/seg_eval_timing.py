"""Timing of the mask-evaluation kernels (sleap_nn_amd/evaluation.py, csrc/eval_kernels.hip).

The case: ``--frames`` frames of ``--size`` x ``--size`` with ``--instances`` ground-truth blobs and as many predicted blobs (each a jittered copy of
its ground-truth blob) per frame, as uint8 mask stacks.  Reported (device events around each call, warmed, median):

* ``ph_mask_pair_stats`` on the two stacks, and on the label-map form of the prediction, with the bytes each reads against the 8 TB/s HBM peak;
* ``boundary_iou`` of the matched pairs: ``ph_mask_boundary`` over both stacks of pairs and ``ph_mask_pair_stats`` with one mask per side (this
  includes the one host read of its result);
* a bare read of the same stack bytes (a torch reduction over them): the floor;
* the project's own host path of the same contract on the same masks (NumPy, wall clock), without any copy.

    python tools/seg_eval_timing.py [--frames 32] [--size 1024] [--instances 16] [--iters 20] [--host-iters 1]
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

from sleap_nn_amd import evaluation as E  # noqa: E402

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


def blobs(B, n, size, seed):
    g = np.random.default_rng(seed)
    gt, pred = np.zeros((B, n, size, size), np.uint8), np.zeros((B, n, size, size), np.uint8)
    for b in range(B):
        for k in range(n):
            cy, cx, ry, rx = g.uniform(60, size - 60), g.uniform(60, size - 60), g.uniform(20, 55), g.uniform(20, 55)
            y0, y1, x0, x1 = int(cy - 64), int(cy + 64), int(cx - 64), int(cx + 64)
            yy, xx = np.mgrid[max(y0, 0) : min(y1, size), max(x0, 0) : min(x1, size)]
            gt[b, k, yy, xx] = ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1
            jy, jx = g.uniform(-4, 4, size=2)
            pred[b, k, yy, xx] = ((yy - cy - jy) / (ry * g.uniform(0.9, 1.1))) ** 2 + ((xx - cx - jx) / (rx * g.uniform(0.9, 1.1))) ** 2 <= 1
    return pred, gt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--instances", type=int, default=16)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--host-iters", type=int, default=1)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("seg_eval_timing needs the GPU")
    dev = "cuda:0"
    B, n, size = args.frames, args.instances, args.size
    pred_h, gt_h = blobs(B, n, size, 11)
    lab_h = np.full((B, size, size), -1, np.int8)
    for k in range(n - 1, -1, -1):
        lab_h[pred_h[:, k] != 0] = k
    pred, gt, lab = torch.from_numpy(pred_h).to(dev), torch.from_numpy(gt_h).to(dev), torch.from_numpy(lab_h).to(dev)
    counts = np.full(B, n)

    # matched pairs (the matching itself is host work on B small matrices and is not timed)
    stats = E.mask_pair_stats(pred, gt, counts, counts)
    ib, ip, ig = [], [], []
    for b, (iou, _, _, _) in enumerate(stats):
        mp, mg = E.match_masks(iou, 0.5)[:2]
        ib += [b] * len(mp)
        ip += list(mp)
        ig += list(mg)
    tb, tp, tg = (torch.as_tensor(np.asarray(v), dtype=torch.long, device=dev) for v in (ib, ip, ig))
    pm, gm = pred[tb, tp].contiguous(), gt[tb, tg].contiguous()
    n_pairs = len(ib)

    for _ in range(3):  # warm up every shape
        E.mask_pair_tables(pred, gt, counts, counts)
        E.mask_pair_tables(lab, gt, counts, counts)
        E.boundary_iou(pm, gm)
        (pred.view(torch.int64).sum() + gt.view(torch.int64).sum()).item()
    t_stack = median_event_us(lambda: E.mask_pair_tables(pred, gt, counts, counts), args.iters)
    t_label = median_event_us(lambda: E.mask_pair_tables(lab, gt, counts, counts), args.iters)
    t_biou = median_event_us(lambda: E.boundary_iou(pm, gm), args.iters)
    t_read = median_event_us(lambda: pred.view(torch.int64).sum() + gt.view(torch.int64).sum(), args.iters)
    by_stack, by_label = pred.numel() + gt.numel(), lab.numel() + gt.numel()
    print(f"case: {B} frames of {size} x {size}, {n} predicted and {n} ground-truth masks per frame, {n_pairs} matched pairs, boundary width d = {E.boundary_width(size, size)}")
    print(f"ph_mask_pair_stats, mask stacks: {t_stack:.1f} us, {by_stack / 1e6:.0f} MB -> {by_stack / t_stack / 1e3:.0f} GB/s = {by_stack / (t_stack * 1e-6) / HBM_PEAK:.3f} of 8 TB/s")
    print(f"ph_mask_pair_stats, label map + ground-truth stack: {t_label:.1f} us, {by_label / 1e6:.0f} MB -> {by_label / t_label / 1e3:.0f} GB/s")
    print(f"bare read of the two stacks (torch sum over int64 views): {t_read:.1f} us -> {by_stack / t_read / 1e3:.0f} GB/s")
    print(f"boundary_iou of the {n_pairs} matched pairs (pad/cat, ph_mask_boundary on {2 * n_pairs} masks, ph_mask_pair_stats, host read): {t_biou:.1f} us")

    def wall(fn, iters):
        ts = []
        for _ in range(iters):
            t = time.perf_counter()
            fn()
            ts.append((time.perf_counter() - t) * 1e6)
        return statistics.median(ts)

    pm_h, gm_h = pm.cpu().numpy(), gm.cpu().numpy()
    h_stack = wall(lambda: E.mask_pair_tables(pred_h, gt_h, counts, counts), args.host_iters)
    h_biou = wall(lambda: E.boundary_iou(pm_h, gm_h), args.host_iters)
    same = all(np.array_equal(a.cpu().numpy(), b) for a, b in zip(E.mask_pair_tables(pred, gt, counts, counts), E.mask_pair_tables(pred_h, gt_h, counts, counts)))
    same_b = np.array_equal(E.boundary_iou(pm, gm), E.boundary_iou(pm_h, gm_h))
    print(f"host path (NumPy, wall clock, masks already on the host): pair tables {h_stack / 1e3:.1f} ms, boundary_iou {h_biou / 1e3:.1f} ms; "
          f"tables identical: {same}, boundary IoUs identical: {same_b}")


if __name__ == "__main__":
    main()
