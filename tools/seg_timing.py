"""Timing of the segmentation grouping stage (sleap_nn_amd/inference/ops/segmentation.py, csrc/seg_kernels.hip).

The case: 8 frames of 256 x 256 head maps (cfg2's 512 x 512 input at output stride 2): foreground, centre and two offset channels,
``--instances`` synthetic instances per frame (Gaussian centre peaks, disks of foreground, offsets towards the centre plus noise).
Reported (device events around each call, warmed, median):

* the grouping launches of one batch -- ``ph_seg_center_peaks`` (two launches), ``ph_seg_assign``, and with ``--gate`` the three
  ``ph_seg_gate`` passes -- each and together, and the algorithmic bytes of the four channels read once plus the label map written
  once against the 8 TB/s HBM peak;
* a bare read of the same four channels' bytes (a torch reduction over them): the floor the peaks kernel is judged against;
* the whole stage end to end (launches + the one host read + building the per-frame masks);
* the host implementation of the same contract on the same maps, including the device-to-host copy of the four channels it needs.

``--plateau N`` puts an N x N plateau of tied maxima into frame 0's centre map: the saturated case, whose candidate list no longer fits LDS and is
propagated by one workgroup in global memory (the launches are then timed at the capacity the retry comes back with).

    python tools/seg_timing.py [--frames 8] [--size 256] [--instances 12] [--gate] [--plateau 0] [--iters 30]
"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from sleap_nn_amd import _lib as L  # noqa: E402
from sleap_nn_amd.inference.ops import segmentation as S  # noqa: E402

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
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t) * 1e6)
    return statistics.median(times)


def synthetic_maps(B, n, size, stride, seed):
    g = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:size, 0:size].astype(np.float32)
    fg = np.full((B, 1, size, size), 0.05, np.float32)
    hm = np.full((B, 1, size, size), 0.01, np.float32)
    off = g.uniform(-8, 8, size=(B, 2, size, size)).astype(np.float32)
    for b in range(B):
        for _ in range(n):
            cx, cy, r = g.uniform(20, size - 20), g.uniform(20, size - 20), g.uniform(10, 22)
            d2 = (xx - cx) ** 2 + (yy - cy) ** 2
            hm[b, 0] = np.maximum(hm[b, 0], g.uniform(0.5, 0.95) * np.exp(-d2 / (2 * 2.0**2)))
            inside = d2 <= r * r
            fg[b, 0][inside] = 0.9
            off[b, 0][inside] = ((cx - xx) * stride + g.normal(0, 0.5, size=xx.shape))[inside]
            off[b, 1][inside] = ((cy - yy) * stride + g.normal(0, 0.5, size=xx.shape))[inside]
    return torch.from_numpy(fg), torch.from_numpy(hm), torch.from_numpy(off)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--instances", type=int, default=12)
    ap.add_argument("--gate", action="store_true")
    ap.add_argument("--plateau", type=int, default=0, help="side of a square plateau of tied maxima put into frame 0's centre map (the saturated case: its candidates exceed the LDS list)")
    ap.add_argument("--iters", type=int, default=30)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("seg_timing needs the GPU")
    dev = "cuda:0"
    B, h, stride = args.frames, args.size, 2
    fg_h, hm_h, off_h = synthetic_maps(B, args.instances, h, stride, 7)
    if args.plateau:
        hm_h[0, 0, 8 : 8 + args.plateau, 8 : 8 + args.plateau] = 0.97
    fg, hm, off = fg_h.to(dev), hm_h.to(dev), off_h.to(dev)
    alpha, iters = (2.0, 3) if args.gate else (None, 0)
    kw = dict(fg_threshold=0.5, peak_threshold=0.2, output_stride=stride, max_instances=None, center_nms_kernel=3, distance_gate_alpha=alpha, distance_gate_iters=3)

    lib, P, st = L.lib(), (lambda t: C.c_void_p(t.data_ptr())), L.current_stream_ptr()
    mc, cap = S.DEFAULT_MAX_CENTERS, max(S.DEFAULT_CAP, args.plateau * args.plateau + 4096 if args.plateau else 0)  # (with a plateau: the capacity the retry would come back with)
    counts = torch.zeros(2 * B, dtype=torch.int32, device=dev)
    cen = torch.zeros(2 * B * mc, dtype=torch.int32, device=dev)
    sc = torch.zeros(B * mc, dtype=torch.float32, device=dev)
    pix = torch.zeros((iters + 1) * B * mc, dtype=torch.int32, device=dev)
    need = int(lib.ph_seg_scratch_bytes(B, h, h, cap))
    scratch = torch.empty((need + 7) // 8, dtype=torch.int64, device=dev)
    labels = torch.empty((B, h, h), dtype=torch.int8, device=dev)
    gated = torch.empty_like(labels)
    dist = torch.empty((B, h, h), dtype=torch.float32, device=dev)

    def peaks():
        L.check(lib.ph_seg_center_peaks(P(hm), B, h, h, 0.2, 3, 0, cap, mc, P(cen), P(sc), P(counts), P(pix), iters + 1, P(scratch), need, st))

    def assign():
        L.check(lib.ph_seg_assign(P(fg), P(off), B, h, h, 0.5, stride, P(cen), P(counts), mc, 1, P(labels), P(dist) if args.gate else None, P(pix), st))

    def gate():
        L.check(lib.ph_seg_gate(P(labels), P(dist), B, h, h, alpha, stride, iters, P(counts), mc, 1, P(pix), P(gated), st))

    def launches():
        peaks()
        assign()
        if args.gate:
            gate()

    for _ in range(3):
        launches()
    torch.cuda.synchronize()
    n_cen = counts[:B].cpu().tolist()
    print(f"{B} frames of {h} x {h} maps, stride {stride}: centres per frame {n_cen}, candidates {counts[B:].cpu().tolist()}, foreground {float((fg > 0.5).float().mean()):.2f}"
          f"{', distance gate alpha 2.0 x 3 passes' if args.gate else ''}")
    t_p, t_a = median_event_us(peaks, args.iters), median_event_us(assign, args.iters)
    t_g = median_event_us(gate, args.iters) if args.gate else 0.0
    t_all = median_event_us(launches, args.iters)
    n_launch = 3 + iters
    bytes_all = 4 * 4 * B * h * h + B * h * h
    print(f"ph_seg_center_peaks (2 launches): {t_p:.1f} us; ph_seg_assign: {t_a:.1f} us" + (f"; ph_seg_gate ({iters} launches): {t_g:.1f} us" if args.gate else ""))
    print(f"the {n_launch} grouping launches of a batch: {t_all:.1f} us; {bytes_all / 1e6:.2f} MB (four channels read once + one-byte labels written) -> "
          f"{bytes_all / (t_all * 1e-6) / 1e9:.0f} GB/s = {bytes_all / (t_all * 1e-6) / HBM_PEAK:.3f} of 8 TB/s")

    four = torch.cat([fg, hm, off], dim=1).contiguous()

    def bare_read():
        return four.sum()

    for _ in range(3):
        bare_read()
    t_r = median_event_us(bare_read, args.iters)
    print(f"bare read of the four channels ({four.numel() * 4 / 1e6:.2f} MB, torch sum): {t_r:.1f} us")

    def device_stage():
        g = S.group_instances_from_offsets(fg, hm, off, **kw)
        return [g.instances(b, stride) for b in range(B)]

    def host_stage():
        g = S.group_instances_from_offsets(fg.cpu(), hm.cpu(), off.cpu(), **kw)
        return [g.instances(b, stride) for b in range(B)]

    d_inst, h_inst = device_stage(), host_stage()
    same = all(len(a) == len(b) and all(np.array_equal(x["mask"], y["mask"]) and x["score"] == y["score"] for x, y in zip(a, b)) for a, b in zip(d_inst, h_inst))
    t_d = median_wall_us(device_stage, max(5, args.iters // 3))
    t_h = median_wall_us(host_stage, max(3, args.iters // 10))
    print(f"stage end to end (launches + one host read + per-instance masks from the label map): {t_d:.0f} us per batch")
    print(f"host implementation on the same maps (D2H of four channels + torch / numpy grouping): {t_h:.0f} us per batch; the device stage is {t_h / t_d:.1f} x faster; "
          f"results identical: {same}")


if __name__ == "__main__":
    main()
