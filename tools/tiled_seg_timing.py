"""Timing of tiled segmentation inference (sleap_nn_amd/inference/layers/tiled.py: TiledSegmentationLayer, ph_tile_merge_heads).

The case: one 4096 x 4096 single-channel uint8 frame, a bottom-up segmentation UNet (f16 / r2 / max_stride 16, synthetic weights) at output stride 2,
tile 512, overlap 128, ``tile_batch_size`` 8.  Reported:

* ``ph_tile_merge_heads`` (one launch: foreground 1 + centre 1 + offset 2 channels) against the composition it replaces, three ``ph_tile_merge`` launches with
  N = 1, 1, 2 on the SAME arenas: device-event medians, taken in alternation ``--repeats`` times so that the spread between repeated medians of the baseline
  is on the page; algorithmic bytes (the arenas read once + the stitched maps written once; the window is not counted) per second against the 8 TB/s HBM
  peak; and whether the two give the same bits;
* ``TiledSegmentationLayer.predict`` split into forward (extract + tile batches + copies into the arenas), stitch and grouping (``inner.postprocess``).  The
  weights are synthetic, so the centre threshold is placed from the stitched centre map itself (just under its ``--centres``-th largest value): the grouping
  then has a bounded number of centres to assign the foreground to.

    python tools/tiled_seg_timing.py [--size 4096] [--tile 512] [--overlap 128] [--iters 20] [--repeats 3] [--no-layer]
"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from benchlegs.single_instance import SI_BB  # noqa: E402
from sleap_nn_amd import _lib as L  # noqa: E402

HBM_PEAK = 8.0e12
HEADS = {"segmentation": {"output_stride": 2, "loss_weight": 1.0, "bce_weight": 1.0, "dice_weight": 1.0},
         "center": {"sigma": 4.0, "output_stride": 2, "loss_weight": 1.0}, "offsets": {"output_stride": 2, "loss_weight": 0.1}}


def median_event_ms(fn, iters):
    """Median over ``iters`` of the device time of one ``fn()`` (an event pair around each call)."""
    times = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return statistics.median(times)


def wall_ms(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3, r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--tile", type=int, default=512)
    ap.add_argument("--overlap", type=int, default=128)
    ap.add_argument("--tile-batch", type=int, default=8)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--centres", type=int, default=32)
    ap.add_argument("--no-layer", action="store_true", help="the two stitches only")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tiled_seg_timing needs the GPU")
    from sleap_nn_amd.architectures.model import Model
    from sleap_nn_amd.inference.backends import HipBackend
    from sleap_nn_amd.inference.layers import PostprocessConfig, SegmentationLayer, TiledSegmentationLayer

    dev = "cuda:0"
    S, ts = args.size, args.tile
    model = Model("unet", SI_BB, HEADS, "bottomup_segmentation").init_xavier_(seed=1234, head_scale=0.05)
    backend = HipBackend(model, dev, use_graph=True)
    make = lambda thr: TiledSegmentationLayer(SegmentationLayer(backend, 2, max_stride=SI_BB["max_stride"], max_instances=args.centres,
                                                                postprocess_config=PostprocessConfig(peak_threshold=thr)), ts, args.overlap, tile_batch_size=args.tile_batch)
    layer = make(0.2)
    frame = torch.randint(0, 256, (1, 1, S, S), dtype=torch.uint8, generator=torch.Generator().manual_seed(4321)).to(dev)

    ys, xs, ys_dev, xs_dev, ys_out, xs_out = layer._grid((S, S))
    ny, nx, stride = len(ys), len(xs), layer.output_stride
    T, t, h = ny * nx, ts // stride, S // stride
    _win_host, win = layer._get_window((t, t))
    channels = (1, 1, 2)
    print(f"frame {S} x {S} uint8, tile {ts} / overlap {args.overlap} -> {ny} x {nx} = {T} tiles, maps (1 + 1 + 2) x {h} x {h}, mean coverage k = {T * t * t / (h * h):.2f}; "
          f"arenas {T * 4 * t * t * 4 / 1e6:.0f} MB, stitched maps {4 * h * h * 4 / 1e6:.0f} MB", flush=True)

    lib, P, stream = L.lib(), (lambda x: C.c_void_p(x.data_ptr())), L.current_stream_ptr()
    g = torch.Generator().manual_seed(99)
    arenas = [torch.randn((T, c, t, t), generator=g).to(dev) for c in channels]
    outs_a = [torch.empty((1, c, h, h), dtype=torch.float32, device=dev) for c in channels]
    outs_b = [torch.empty((1, c, h, h), dtype=torch.float32, device=dev) for c in channels]
    ap_, op_, ch_ = (C.c_void_p * 3)(*[a.data_ptr() for a in arenas]), (C.c_void_p * 3)(*[o.data_ptr() for o in outs_b]), (C.c_int32 * 3)(*channels)

    def three_launches():
        for a, o, c in zip(arenas, outs_a, channels):
            L.check(lib.ph_tile_merge(P(a), P(win), 1, c, t, t, P(ys_out), ny, P(xs_out), nx, h, h, P(o), stream))

    def one_launch():
        L.check(lib.ph_tile_merge_heads(ap_, ch_, 3, P(win), 1, t, t, P(ys_out), ny, P(xs_out), nx, h, h, op_, stream))

    for _ in range(3):
        three_launches()
        one_launch()
    torch.cuda.synchronize()
    same = all(bool(torch.equal(a.view(torch.int32), b.view(torch.int32))) for a, b in zip(outs_a, outs_b))
    base, heads = [], []
    for _ in range(args.repeats):
        base.append(median_event_ms(three_launches, args.iters))
        heads.append(median_event_ms(one_launch, args.iters))
    nbytes = 4 * (sum(a.numel() for a in arenas) + sum(o.numel() for o in outs_a))
    rate = lambda ms: f"{nbytes / (ms * 1e-3) / 1e9:.0f} GB/s = {nbytes / (ms * 1e-3) / HBM_PEAK:.2f} of 8 TB/s"
    b_med, h_med = statistics.median(base), statistics.median(heads)
    print(f"3 x ph_tile_merge (N = 1, 1, 2): medians of {args.repeats} runs of {args.iters}: {[round(v * 1e3, 1) for v in base]} us -> {b_med * 1e3:.1f} us "
          f"(spread {(max(base) - min(base)) * 1e3:.1f} us), {nbytes / 1e6:.0f} MB -> {rate(b_med)}")
    print(f"ph_tile_merge_heads (one launch): {[round(v * 1e3, 1) for v in heads]} us -> {h_med * 1e3:.1f} us (spread {(max(heads) - min(heads)) * 1e3:.1f} us), "
          f"{nbytes / 1e6:.0f} MB -> {rate(h_med)}; {b_med / h_med:.2f} x the three launches' speed; results bit-identical: {same}", flush=True)
    if args.no_layer:
        return

    # the layer: forward / stitch / grouping.  The centre threshold comes from the stitched centre map (synthetic weights).
    raw_out, _info = layer._stitch(frame)
    cen = raw_out[layer.inner._CENTER_KEY].flatten()
    thr = float(torch.topk(cen, 4 * args.centres).values[-1])
    fg_frac = float((raw_out[layer.inner._SEG_KEY] > 0.5).float().mean())
    layer = make(thr)
    layer.inner.fg_threshold = float(torch.quantile(raw_out[layer.inner._SEG_KEY].flatten()[:: max(1, cen.numel() // 1_000_000)], 0.7))  # ~30 % foreground
    print(f"centre threshold {thr:.4f} (the {4 * args.centres}-th largest stitched centre value), at most {args.centres} centres kept; foreground threshold "
          f"{layer.inner.fg_threshold:.4f} (was {fg_frac:.2f} of the pixels above 0.5)", flush=True)
    from sleap_nn_amd.inference.tile_merger import extract_tiles, merge_tile_heads

    keys = layer._head_keys()

    def forward():
        tiles = extract_tiles(frame, ys_dev, xs_dev, ts)
        ar = [torch.empty((T, c, t, t), dtype=torch.float32, device=dev) for c in channels]
        for i in range(0, T, args.tile_batch):
            chunk = tiles[i : i + args.tile_batch]
            with torch.inference_mode():
                raw = backend(chunk.unsqueeze(1))
            for a, k in zip(ar, keys):
                a[i : i + chunk.shape[0]].copy_(raw[k])
        return ar

    reps = max(3, args.iters // 4)
    forward()
    f_ms, ar = zip(*[wall_ms(forward) for _ in range(reps)])
    ar = ar[-1]
    s_ms, heads_out = zip(*[wall_ms(lambda: merge_tile_heads(ar, win, ys_out, xs_out, (h, h))) for _ in range(reps)])
    raw_out, info = layer._stitch(frame)
    g_ms, res = zip(*[wall_ms(lambda: layer.inner.postprocess(raw_out, info)) for _ in range(reps)])
    p_ms, _ = zip(*[wall_ms(lambda: layer.predict(frame)) for _ in range(reps)])
    med = statistics.median
    print(f"TiledSegmentationLayer.predict: {med(p_ms):.2f} ms per frame = forward of {T} tiles in chunks of {args.tile_batch} (+ extract, copies into the arenas) "
          f"{med(f_ms):.2f} ms + stitch {med(s_ms):.3f} ms + grouping {med(g_ms):.2f} ms ({len(res[-1].pred_masks[0])} instances); wall clock, medians of {reps}")


if __name__ == "__main__":
    main()
