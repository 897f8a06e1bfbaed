"""Timing of the class-map target rendering (sleap_nn_amd/data/targets.py, csrc/target_kernels.hip).

The case: BASELINE cfg5's shape -- 16 frames of 768 x 768, 4 animals (one per class) of 17 nodes each, class maps at output stride 8 with
sigma 12.5 (benchlegs/infer_cfg5.py) -- or whatever ``--size / --batch / --instances / --nodes / --classes / --stride`` say.
Reported (device events around each call, warmed, median):

* ``ph_render_class_maps``: the one launch of a batch, with the bytes it writes (the (B, C, h, w) output; its input is a few KiB) and the
  Gaussians it evaluates (two sweeps: I for the sum, one per non-zero weight for the masks);
* the torch composition of the same functions on the device (``targets._class_maps_torch`` on device tensors: the (B, I, N, h, w)
  Gaussians, their maximum over the nodes, the sum, the mask, the weighted maximum), and the largest difference between the two results;
* ``generate_class_maps`` end to end from device points and class indices (weight matrix + launch), which is what a training loop calls.

    python tools/targets_timing.py [--size 768] [--batch 16] [--instances 4] [--nodes 17] [--classes 4] [--stride 8] [--sigma 12.5] [--iters 50]
"""
import argparse
import ctypes as C
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from sleap_nn_amd import _lib as L  # noqa: E402
from sleap_nn_amd.data import targets as T  # noqa: E402


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=768)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--instances", type=int, default=4)
    ap.add_argument("--nodes", type=int, default=17)
    ap.add_argument("--classes", type=int, default=4)
    ap.add_argument("--stride", type=int, default=8)
    ap.add_argument("--sigma", type=float, default=12.5)
    ap.add_argument("--threshold", type=float, default=0.2)
    ap.add_argument("--iters", type=int, default=50)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("targets_timing needs the GPU")
    dev = "cuda:0"
    S, B, I, N, K = args.size, args.batch, args.instances, args.nodes, args.classes
    rng = np.random.RandomState(3)
    pts_h = np.stack([np.clip(rng.uniform(120, S - 120, size=(I, 1, 2)) + rng.normal(0, 35, size=(I, N, 2)), 6, S - 7) for _ in range(B)]).astype(np.float32)
    pts = torch.from_numpy(pts_h).to(dev)
    cls = torch.from_numpy(np.stack([rng.permutation(max(I, K))[:I] % K for _ in range(B)]).astype(np.int32)).to(dev)
    wts = T.class_map_weights(cls, K).contiguous()
    h = w = (S + args.stride - 1) // args.stride
    out = torch.empty((B, K, h, w), dtype=torch.float32, device=dev)
    lib, P, st = L.lib(), (lambda t: C.c_void_p(t.data_ptr())), L.current_stream_ptr()

    def kernel():
        L.check(lib.ph_render_class_maps(P(pts), P(wts), B, I, N, K, S, S, args.stride, args.sigma, args.threshold, P(out), st))

    def composition():
        return T._class_maps_torch(pts, wts, (S, S), args.threshold, args.sigma, args.stride)

    def end_to_end():
        return T.generate_class_maps(pts, (S, S), cls, K, class_map_threshold=args.threshold, sigma=args.sigma, output_stride=args.stride)

    for _ in range(5):
        kernel()
        ref = composition()
        end_to_end()
    torch.cuda.synchronize()
    diff = float((out - ref).abs().max())
    t_k, t_c, t_e = median_event_us(kernel, args.iters), median_event_us(composition, args.iters), median_event_us(end_to_end, args.iters)
    nnz = int((wts != 0).sum())
    gauss = h * w * (B * I + nnz)  # sweep 1: every instance; sweep 2: one per non-zero weight
    print(f"{B} frames of {S} x {S}, {I} instances x {N} nodes, {K} classes, stride {args.stride} (maps {h} x {w}), sigma {args.sigma}, threshold {args.threshold}")
    print(f"ph_render_class_maps: {t_k:.1f} us per batch; writes {out.numel() * 4 / 1e6:.2f} MB, evaluates {gauss / 1e6:.2f} M instance maps of {N} nodes "
          f"({gauss * N / (t_k * 1e-6) / 1e9:.1f} G node distances / s)")
    print(f"torch composition on the device: {t_c:.1f} us per batch ({t_c / t_k:.1f} x the kernel); largest difference between the two results {diff:.2e}")
    print(f"generate_class_maps end to end (weight matrix + launch): {t_e:.1f} us per batch")


if __name__ == "__main__":
    main()
