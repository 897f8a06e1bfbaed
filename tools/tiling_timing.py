"""Timing of tiled single-instance inference (sleap_nn_amd/inference/layers/tiled.py, ph_tile_extract / ph_tile_merge).

The case: one 4096 x 4096 single-channel uint8 frame, a 13-node single-instance UNet (f16 / r2 / max_stride 16, synthetic weights)
at output stride 2, tile 512, overlap 128, ``tile_batch_size`` 8.  Reported:

* per-launch time of ``ph_tile_extract`` and ``ph_tile_merge`` (device events around each launch, warmed, median), and their
  algorithmic bytes per second against the 8 TB/s HBM peak: extract = tile elements read once + written once, merge = tile-map
  elements read once + the stitched maps written once (the window is not counted);
* the forward of the tile batches (hipGraph replay per chunk) and the whole ``predict``;
* on the same device and the same tile maps, the reference's scatter algorithm -- the torch ``TileMerger`` with ``device="cuda"``:
  per tile ``ACC[...] += tile * w``, ``CNT[...] += w``, then one divide -- which is what one would write without the kernel.

    python tools/tiling_timing.py [--size 4096] [--tile 512] [--overlap 128] [--iters 20]
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
from sleap_nn_amd.inference.tile_merger import TileMerger  # noqa: E402

HBM_PEAK = 8.0e12


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


def median_wall_ms(fn, iters):
    times = []
    for _ in range(iters):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t) * 1e3)
    return statistics.median(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--tile", type=int, default=512)
    ap.add_argument("--overlap", type=int, default=128)
    ap.add_argument("--nodes", type=int, default=13)
    ap.add_argument("--tile-batch", type=int, default=8)
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tiling_timing needs the GPU")
    from sleap_nn_amd.architectures.model import Model
    from sleap_nn_amd.inference.backends import HipBackend
    from sleap_nn_amd.inference.layers import PostprocessConfig, SingleInstanceLayer, TiledLayer

    dev = "cuda:0"
    S, ts, N = args.size, args.tile, args.nodes
    heads = {"confmaps": {"part_names": [f"k{i}" for i in range(N)], "sigma": 2.5, "output_stride": 2, "loss_weight": 1.0}}
    model = Model("unet", SI_BB, heads, "single_instance").init_xavier_(seed=1234, head_scale=0.05)
    inner = SingleInstanceLayer(HipBackend(model, dev, use_graph=True), 2, max_stride=SI_BB["max_stride"], postprocess_config=PostprocessConfig(peak_threshold=0.0))
    layer = TiledLayer(inner, ts, args.overlap, tile_batch_size=args.tile_batch)
    frame = torch.randint(0, 256, (1, 1, S, S), dtype=torch.uint8, generator=torch.Generator().manual_seed(4321)).to(dev)

    ys, xs, ys_dev, xs_dev, ys_out, xs_out = layer._grid((S, S))
    ny, nx, stride = len(ys), len(xs), layer.output_stride
    T, t, h = ny * nx, ts // stride, S // stride
    win_host, win = layer._get_window((t, t))
    cover = T * t * t / (h * h)
    print(f"frame {S} x {S} uint8, tile {ts} / overlap {args.overlap} -> {ny} x {nx} = {T} tiles (step {xs[1] - xs[0] if nx > 1 else 0}), maps {N} x {h} x {h}, "
          f"mean coverage k = {cover:.2f}; tile-map arena {T * N * t * t * 4 / 1e6:.0f} MB, stitched maps {N * h * h * 4 / 1e6:.0f} MB")

    lib, P, stream = L.lib(), (lambda x: C.c_void_p(x.data_ptr())), L.current_stream_ptr()
    tiles = torch.empty((T, 1, ts, ts), dtype=torch.uint8, device=dev)

    def extract():
        L.check(lib.ph_tile_extract(P(frame), 0, 1, 1, S, S, P(ys_dev), ny, P(xs_dev), nx, ts, P(tiles), stream))

    for _ in range(3):
        extract()
    e_ms = median_event_ms(extract, args.iters)
    e_bytes = 2 * tiles.numel()
    print(f"ph_tile_extract: {e_ms * 1e3:.1f} us per launch, {e_bytes / 1e6:.1f} MB -> {e_bytes / (e_ms * 1e-3) / 1e9:.0f} GB/s = {e_bytes / (e_ms * 1e-3) / HBM_PEAK:.2f} of 8 TB/s")

    # the forward of the tile batches: the chunks of predict(), each one replay of the captured graph
    arena = torch.empty((T, N, t, t), dtype=torch.float32, device=dev)

    def forward():
        for i in range(0, T, args.tile_batch):
            chunk = tiles[i : i + args.tile_batch]
            arena[i : i + chunk.shape[0]].copy_(inner._extract_confmaps(inner.backend(chunk.unsqueeze(1))))

    forward()
    forward()
    f_ms = median_wall_ms(forward, max(3, args.iters // 4))
    print(f"forward of {T} tiles in chunks of {args.tile_batch} (+ copy into the arena): {f_ms:.2f} ms")

    out = torch.empty((1, N, h, h), dtype=torch.float32, device=dev)

    def merge():
        L.check(lib.ph_tile_merge(P(arena), P(win), 1, N, t, t, P(ys_out), ny, P(xs_out), nx, h, h, P(out), stream))

    for _ in range(3):
        merge()
    m_ms = median_event_ms(merge, args.iters)
    m_bytes = 4 * (arena.numel() + out.numel())
    print(f"ph_tile_merge: {m_ms * 1e3:.1f} us per launch, {m_bytes / 1e6:.0f} MB -> {m_bytes / (m_ms * 1e-3) / 1e9:.0f} GB/s = {m_bytes / (m_ms * 1e-3) / HBM_PEAK:.2f} of 8 TB/s")

    origins = [(y // stride, x // stride) for y in ys for x in xs]

    def scatter():
        m = TileMerger((h, h), N, win, device=dev)
        for k, (y0, x0) in enumerate(origins):
            m.integrate(arena[k], y0, x0)
        return m.merge()

    for _ in range(2):
        ref = scatter()
    s_ms = median_event_ms(scatter, args.iters)
    same = bool(torch.equal(ref.view(torch.int32), out[0].view(torch.int32)))
    print(f"torch TileMerger on the device (scatter, {2 * T + 1} passes over tile- or canvas-sized tensors): {s_ms * 1e3:.1f} us; "
          f"ph_tile_merge is {s_ms / m_ms:.1f} x faster; results bit-identical: {same}")

    layer.predict(frame)
    p_ms = median_wall_ms(lambda: layer.predict(frame), max(3, args.iters // 4))
    print(f"TiledLayer.predict (preprocess + extract + {-(-T // args.tile_batch)} forwards + merge + global peaks): {p_ms:.2f} ms per frame")


if __name__ == "__main__":
    main()
