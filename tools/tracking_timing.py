"""Timing of the tracker (``sleap_nn_amd/tracking``): per-frame cost of ``Tracker.track_outputs`` with the pair tables against the same tracker scoring pair
by pair on the host, on batches of 8 frames with 12 instances, at windows 5 and 25.  Reported (warmed, median over ``--iters`` runs of ``--batches`` batches):

* poses (12 instances of 13 nodes on slow paths, 10 % missing nodes): ``ph_track_pose_scores`` (csrc/track_host.cpp) against the NumPy scores;
* masks (256 x 256 maps at stride 2, 12 discs, through ``SegmentationLayer.postprocess`` on the device): ``ph_track_mask_pairs`` (csrc/track_kernels.hip, the device
  ring, one device-to-host copy per batch) against the host scoring on the ``pred_masks`` arrays (every mask decoded to the image grid, one crop AND per pair);
* the ``ph_track_mask_pairs`` launch alone (device events) with the bytes it reads.

    python tools/tracking_timing.py [--frames 8] [--size 256] [--instances 12] [--batches 6] [--iters 5]
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402
from seg_timing import median_event_us  # noqa: E402

from sleap_nn_amd.inference.outputs import Outputs  # noqa: E402
from sleap_nn_amd.tracking import Tracker  # noqa: E402
from sleap_nn_amd.tracking import scoring as S  # noqa: E402


def pose_batches(n_batches, B, n_inst, n_nodes, seed):
    g = np.random.default_rng(seed)
    pos = g.uniform(50, 950, (n_inst, 2))
    vel = g.normal(0, 3, (n_inst, 2))
    shape = g.normal(0, 15, (n_inst, n_nodes, 2))
    out = []
    for k in range(n_batches):
        kp = np.zeros((B, n_inst, n_nodes, 2), np.float32)
        for b in range(B):
            vel = 0.9 * vel + g.normal(0, 1.0, vel.shape)
            pos = pos + vel
            pts = pos[:, None] + shape + g.normal(0, 0.8, shape.shape)
            pts[g.uniform(size=pts.shape[:2]) < 0.1] = np.nan
            kp[b] = pts[g.permutation(n_inst)]
        out.append(Outputs(pred_keypoints=torch.from_numpy(kp), instance_scores=torch.rand(B, n_inst), frame_indices=torch.arange(k * B, (k + 1) * B)))
    return out


def disc_maps(n_batches, B, n_inst, size, stride, seed):
    g = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:size, 0:size].astype(np.float32)
    pos = g.uniform(25, size - 25, (n_inst, 2))
    vel = g.normal(0, 1.5, (n_inst, 2))
    rad = g.uniform(9, 16, n_inst)
    out = []
    for _k in range(n_batches):
        fg = np.full((B, 1, size, size), 0.05, np.float32)
        hm = np.full((B, 1, size, size), 0.01, np.float32)
        off = np.zeros((B, 2, size, size), np.float32)
        for b in range(B):
            vel = 0.9 * vel + g.normal(0, 0.5, vel.shape)
            pos = np.clip(pos + vel, 20, size - 20)
            for a in range(n_inst):
                cx, cy = np.round(pos[a])
                d2 = (xx - cx) ** 2 + (yy - cy) ** 2
                hm[b, 0] = np.maximum(hm[b, 0], 0.9 * np.exp(-d2 / (2 * 2.0**2)))
                inside = d2 <= rad[a] ** 2
                fg[b, 0][inside] = 0.9
                off[b, 0][inside] = ((cx - xx) * stride)[inside]
                off[b, 1][inside] = ((cy - yy) * stride)[inside]
        out.append((torch.from_numpy(fg), torch.from_numpy(hm), torch.from_numpy(off)))
    return out


def per_frame_us(make_tracker, batches, use_tables, iters):
    times = []
    for _ in range(iters + 1):
        tr = make_tracker()
        torch.cuda.synchronize()
        t = time.perf_counter()
        for o in batches:
            tr.track_outputs(o, use_tables=use_tables)
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t) * 1e6 / sum(o.batch_size for o in batches))
    return statistics.median(times[1:]), tr


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--instances", type=int, default=12)
    ap.add_argument("--batches", type=int, default=6)
    ap.add_argument("--iters", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tracking_timing needs the GPU")
    dev = "cuda:0"
    B, n = args.frames, args.instances
    print(f"{args.batches} batches of {B} frames, {n} instances per frame; per-frame tracker cost, median of {args.iters} runs")

    poses = pose_batches(args.batches, B, n, 13, 3)
    for window in (5, 25):
        mk = lambda w=window: Tracker.from_config(window_size=w)
        t_native, tr = per_frame_us(mk, poses, True, args.iters)
        t_numpy, _ = per_frame_us(mk, poses, False, args.iters)
        print(f"poses, oks, window {window}: native scores {t_native:.0f} us/frame ({tr.table_hits} scores from the table, {tr.pair_calls} pair by pair), "
              f"NumPy scores {t_numpy:.0f} us/frame -> x{t_numpy / t_native:.1f}")

    from sleap_nn_amd.inference.layers.segmentation import SegmentationLayer
    from sleap_nn_amd.inference.preprocess_info import PreprocInfo

    class _Backend:  # the layer's postprocess is driven directly: no forward
        device, does_baked_postproc, model = dev, False, None

        def __call__(self, x):
            raise RuntimeError("no forward in this tool")

        def warmup(self, input_shape):
            pass

    stride = 2
    layer = SegmentationLayer(_Backend(), stride, keep_label_map=True)
    info = PreprocInfo(original_size=(args.size * stride, args.size * stride), processed_size=(args.size * stride, args.size * stride), eff_scale=torch.ones(B), input_scale=1.0,
                       output_stride=stride)
    outs = []
    for k, (fg, hm, off) in enumerate(disc_maps(args.batches, B, n, args.size, stride, 5)):
        o = layer.postprocess({"SegmentationHead": fg.to(dev), "InstanceCenterHead": hm.to(dev), "CenterOffsetHead": off.to(dev)}, info)
        o.frame_indices = torch.arange(k * B, (k + 1) * B)
        outs.append(o)
    print(f"masks per frame: {[len(f) for f in outs[0].pred_masks]} (first batch), label map {tuple(outs[0].pred_label_map.shape)} {outs[0].pred_label_map.dtype}")
    for window in (5, 25):
        mk = lambda w=window: Tracker.from_config(window_size=w, features="masks", scoring_method="mask_iou")
        t_dev, tr = per_frame_us(mk, outs, True, args.iters)
        t_host, _ = per_frame_us(mk, outs, False, args.iters)
        print(f"masks, mask_iou, window {window}: device tables {t_dev:.0f} us/frame ({tr.table_hits} scores from the tables, {tr.pair_calls} pair by pair), "
              f"host scoring {t_host:.0f} us/frame -> x{t_host / t_dev:.1f}")
        lm = outs[0].pred_label_map
        L = min(window, S.MAX_TABLE_LAGS)
        ring = torch.cat([o.pred_label_map for o in outs])[-L:].contiguous()
        rw, cw = (torch.from_numpy(a).to(dev) for a in outs[0].pred_label_weights[0])
        px = int(rw.sum()) * int(cw.sum())
        t_k = median_event_us(lambda: S.mask_pair_counts(lm, ring, L, rw, cw, 16, px), 30)
        nbytes = 2 * B * L * lm[0].numel() * lm.element_size()
        print(f"  ph_track_mask_pairs alone, B={B} L={L} P=16: {t_k:.1f} us, {nbytes / 1e6:.1f} MB of label reads -> {nbytes / t_k / 1e3:.0f} GB/s")


if __name__ == "__main__":
    main()
