"""Importance windows and the accumulate / normalise stitch of tiled inference (``sleap_nn/inference/tile_merger.py``).

``build_importance_window`` weights a tile's pixels by their distance from its border; ``TileMerger`` is the plain torch
canvas: ``ACC += tile * w``, ``CNT += w`` per tile, ``ACC / CNT`` at the end.  Everything is in output-stride pixels.

``TileMerger`` is the public class of the reference, the ``accumulator_device="cpu"`` path of ``TiledLayer`` and the statement
of the arithmetic that ``ph_tile_merge`` (``csrc/tile_kernels.hip``) reproduces bit for bit as a gather; ``merge_tiles`` is
that kernel's wrapper, ``merge_tile_heads`` the wrapper of ``ph_tile_merge_heads`` (several heads sharing one grid, one launch).
"""
from __future__ import annotations

import ctypes as C
from typing import List, Optional, Sequence, Tuple, Union

import torch

from sleap_nn_amd import _lib as L

BLEND_MODES = ("gaussian", "pyramid", "constant")


def build_importance_window(tile_hw: Tuple[int, int], mode: str = "gaussian", sigma_scale: float = 0.125, device: Union[str, torch.device] = "cpu",
                            dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """``(th, tw)`` window, 1.0 at the centre, floored at 1e-3, not normalised to a sum (the merge divides by the summed weights).

    ``gaussian``: outer product of per-axis Gaussians with std ``sigma_scale * axis length``; ``pyramid``: outer product of
    per-axis triangular ramps (distance to the nearer edge, peak 1); ``constant``: ones.  The float32 statements run on the host
    (one window per tile size; the same rounding wherever the model runs) and the result is moved to ``device``."""
    th, tw = int(tile_hw[0]), int(tile_hw[1])
    if mode == "gaussian":
        axes = []
        for n in (th, tw):
            half = (n - 1) / 2.0
            pos = torch.arange(-half, half + 1)  # n centred coordinates
            axes.append(torch.exp(pos**2 / (-2 * (sigma_scale * n) ** 2)))
        w = axes[0][:, None] * axes[1][None, :]
    elif mode == "pyramid":
        axes = []
        for n in (th, tw):
            k = torch.arange(1, n + 1, dtype=torch.float32)
            ramp = torch.minimum(k, n + 1 - k)
            axes.append(ramp / ramp.max())
        w = axes[0][:, None] * axes[1][None, :]
    elif mode == "constant":
        w = torch.ones((th, tw))
    else:
        raise ValueError(f"Unknown importance window mode: {mode!r}. Expected one of {', '.join(repr(m) for m in BLEND_MODES)}.")
    floor = max(w.min().item(), 1e-3)  # every covered pixel keeps a strictly positive weight
    return torch.clamp(w, min=floor).to(dtype).to(device)


class TileMerger:
    """Per-frame canvas: ``acc (channels, H, W)`` and ``cnt (1, H, W)`` in ``dtype`` (tiles of lower precision are converted
    first), ``w (1, th, tw)``."""

    def __init__(self, out_hw: Tuple[int, int], channels: int, window: torch.Tensor, device: Union[str, torch.device] = "cpu",
                 dtype: torch.dtype = torch.float32) -> None:
        H, W = out_hw
        self.w = window.to(device=device, dtype=dtype)[None]
        self.acc = torch.zeros((channels, H, W), device=device, dtype=dtype)
        self.cnt = torch.zeros((1, H, W), device=device, dtype=dtype)

    def integrate(self, tile: torch.Tensor, y0: int, x0: int) -> None:
        """Add ``tile (channels, th', tw')`` at canvas position ``(y0, x0)``; a tile clipped by the canvas edge (smaller than the
        window) uses the window's top-left part."""
        tile = tile.to(self.acc.device, self.acc.dtype)
        th, tw = tile.shape[-2:]
        w = self.w[:, :th, :tw]
        self.acc[:, y0 : y0 + th, x0 : x0 + tw] += tile * w
        self.cnt[:, y0 : y0 + th, x0 : x0 + tw] += w

    def merge(self, eps: Optional[float] = None) -> torch.Tensor:
        """``acc / cnt`` ``(channels, H, W)``; uncovered pixels are NaN unless ``eps`` floors the divisor."""
        return self.acc / (self.cnt if eps is None else torch.clamp(self.cnt, min=eps))


def merge_tiles(tile_maps: torch.Tensor, window: torch.Tensor, y_origins: Union[torch.Tensor, Sequence[int]], x_origins: Union[torch.Tensor, Sequence[int]],
                out_hw: Tuple[int, int], frames: int = 1) -> torch.Tensor:
    """``ph_tile_merge``: ``tile_maps (frames * ny * nx, N, th, tw)`` fp32 on the GPU (tile ``iy * nx + ix`` of frame ``f`` at row
    ``f * ny * nx + iy * nx + ix``) -> ``(frames, N, h, w)``, bit-identical to integrating the tiles into a ``TileMerger`` in row
    order and cropping ``merge()`` to ``out_hw``.  Origins are per axis, in output-stride pixels (lists, or int32 device tensors)."""
    L.require_cuda(tile_maps, "tile_maps")
    dev = tile_maps.device
    if tile_maps.dim() != 4 or tile_maps.dtype != torch.float32:
        raise ValueError(f"tile_maps must be a float32 (tiles, N, th, tw) tensor, got {tile_maps.dtype} {tuple(tile_maps.shape)}")
    tile_maps = tile_maps.contiguous()
    yo, xo = origins_tensor(y_origins, dev), origins_tensor(x_origins, dev)
    ny, nx = int(yo.numel()), int(xo.numel())
    n_tiles, N, th, tw = tile_maps.shape
    if n_tiles != frames * ny * nx:
        raise ValueError(f"{n_tiles} tile maps for {frames} frames of {ny} x {nx} tiles")
    if tuple(window.shape) != (th, tw):
        raise ValueError(f"window {tuple(window.shape)} does not match the tile maps ({th}, {tw})")
    window = window.to(device=dev, dtype=torch.float32).contiguous()
    h, w = int(out_hw[0]), int(out_hw[1])
    out = torch.empty((frames, N, h, w), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        L.check(L.lib().ph_tile_merge(C.c_void_p(tile_maps.data_ptr()), C.c_void_p(window.data_ptr()), frames, N, th, tw, C.c_void_p(yo.data_ptr()), ny,
                                      C.c_void_p(xo.data_ptr()), nx, h, w, C.c_void_p(out.data_ptr()), L.current_stream_ptr()))
    return out


MERGE_MAX_HEADS = 4  # ``ph_tile_merge_heads``: the pointers travel in the kernel argument
MERGE_MAX_CHANNELS = 8


def merge_tile_heads(arenas: Sequence[torch.Tensor], window: torch.Tensor, y_origins: Union[torch.Tensor, Sequence[int]], x_origins: Union[torch.Tensor, Sequence[int]],
                     out_hw: Tuple[int, int], frames: int = 1) -> List[torch.Tensor]:
    """``ph_tile_merge_heads``: ``K`` arenas ``(frames * ny * nx, c_k, th, tw)`` fp32 on one GPU (1 <= K <= 4, at most 8 channels in total, one window, one
    grid) -> ``K`` contiguous maps ``(frames, c_k, h, w)`` in ONE launch on the current stream; each is bit-identical to ``merge_tiles`` on its arena and to
    the matching channels of one ``TileMerger`` canvas of ``sum c_k`` channels."""
    arenas = list(arenas)
    if not 1 <= len(arenas) <= MERGE_MAX_HEADS:
        raise ValueError(f"merge_tile_heads takes 1 to {MERGE_MAX_HEADS} arenas, got {len(arenas)}")
    for k, a in enumerate(arenas):
        L.require_cuda(a, f"arenas[{k}]")
        if a.dim() != 4 or a.dtype != torch.float32:
            raise ValueError(f"arenas[{k}] must be a float32 (tiles, c, th, tw) tensor, got {a.dtype} {tuple(a.shape)}")
    dev = arenas[0].device
    n_tiles, _c, th, tw = arenas[0].shape
    for k, a in enumerate(arenas):
        if a.device != dev or a.shape[0] != n_tiles or tuple(a.shape[-2:]) != (th, tw):
            raise ValueError(f"arenas[{k}] {tuple(a.shape)} on {a.device} does not match arenas[0] {tuple(arenas[0].shape)} on {dev}")
        if a.shape[1] < 1:
            raise ValueError(f"arenas[{k}] has no channels")
    total = sum(int(a.shape[1]) for a in arenas)
    if total > MERGE_MAX_CHANNELS:
        raise ValueError(f"{total} channels in total, ph_tile_merge_heads takes at most {MERGE_MAX_CHANNELS}")
    arenas = [a.contiguous() for a in arenas]
    yo, xo = origins_tensor(y_origins, dev), origins_tensor(x_origins, dev)
    ny, nx = int(yo.numel()), int(xo.numel())
    if n_tiles != frames * ny * nx:
        raise ValueError(f"{n_tiles} tile maps for {frames} frames of {ny} x {nx} tiles")
    if tuple(window.shape) != (th, tw):
        raise ValueError(f"window {tuple(window.shape)} does not match the tile maps ({th}, {tw})")
    window = window.to(device=dev, dtype=torch.float32).contiguous()
    h, w = int(out_hw[0]), int(out_hw[1])
    outs = [torch.empty((frames, int(a.shape[1]), h, w), dtype=torch.float32, device=dev) for a in arenas]
    merge_tile_heads_into(arenas, window, yo, xo, outs)
    return outs


def merge_tile_heads_into(arenas: Sequence[torch.Tensor], window: torch.Tensor, yo: torch.Tensor, xo: torch.Tensor, outs: Sequence[torch.Tensor]) -> None:
    """The launch of ``merge_tile_heads`` into caller-owned contiguous ``outs (frames, c_k, h, w)`` (views at any 4-byte-aligned address); arguments are taken as
    validated: contiguous fp32 arenas, an fp32 device window, int32 device origins."""
    K = len(arenas)
    frames, _c, h, w = outs[0].shape
    th, tw = arenas[0].shape[-2:]
    for a, o in zip(arenas, outs):
        if not o.is_contiguous() or o.dtype != torch.float32 or tuple(o.shape) != (frames, a.shape[1], h, w) or o.device != a.device:
            raise ValueError(f"output {tuple(o.shape)} {o.dtype} does not match its arena {tuple(a.shape)} (contiguous float32 (frames, c, h, w) expected)")
    ptrs = (C.c_void_p * K)(*[a.data_ptr() for a in arenas])
    optrs = (C.c_void_p * K)(*[o.data_ptr() for o in outs])
    chans = (C.c_int32 * K)(*[int(a.shape[1]) for a in arenas])
    with torch.cuda.device(arenas[0].device):
        L.check(L.lib().ph_tile_merge_heads(ptrs, chans, K, C.c_void_p(window.data_ptr()), int(frames), int(th), int(tw), C.c_void_p(yo.data_ptr()), int(yo.numel()),
                                            C.c_void_p(xo.data_ptr()), int(xo.numel()), int(h), int(w), optrs, L.current_stream_ptr()))


def extract_tiles(frames: torch.Tensor, y_origins: Union[torch.Tensor, Sequence[int]], x_origins: Union[torch.Tensor, Sequence[int]], tile_size: int) -> torch.Tensor:
    """``ph_tile_extract``: ``frames (F, C, H, W)`` uint8 / float32 on the GPU -> ``(F * ny * nx, C, tile_size, tile_size)``, tiles
    in row-major origin order per frame, zeros past the frame's edges.  Origins are per axis, in frame pixels."""
    L.require_cuda(frames, "frames")
    dev = frames.device
    if frames.dim() != 4 or frames.dtype not in (torch.uint8, torch.float32):
        raise ValueError(f"frames must be a uint8 or float32 (F, C, H, W) tensor, got {frames.dtype} {tuple(frames.shape)}")
    frames = frames.contiguous()
    yo, xo = origins_tensor(y_origins, dev), origins_tensor(x_origins, dev)
    ny, nx = int(yo.numel()), int(xo.numel())
    F, Cc, H, W = frames.shape
    ts = int(tile_size)
    out = torch.empty((F * ny * nx, Cc, ts, ts), dtype=frames.dtype, device=dev)
    with torch.cuda.device(dev):
        L.check(L.lib().ph_tile_extract(C.c_void_p(frames.data_ptr()), 0 if frames.dtype == torch.uint8 else 1, F, Cc, H, W, C.c_void_p(yo.data_ptr()), ny,
                                        C.c_void_p(xo.data_ptr()), nx, ts, C.c_void_p(out.data_ptr()), L.current_stream_ptr()))
    return out


def origins_tensor(origins, device) -> torch.Tensor:
    """Per-axis origins as a contiguous int32 tensor on ``device`` (a tensor that already is one is passed through)."""
    if torch.is_tensor(origins):
        if origins.dim() != 1 or origins.numel() == 0:
            raise ValueError(f"origins must be a non-empty 1-D tensor, got shape {tuple(origins.shape)}")
        return origins.to(device=device, dtype=torch.int32).contiguous()
    vals = [int(v) for v in origins]
    if not vals:
        raise ValueError("origins must not be empty")
    return torch.tensor(vals, dtype=torch.int32).to(device)
