"""Tile grid of tiled inference (``sleap_nn/data/tiling.py``: ``generate_tile_grid``).

Pure Python: the origins of the overlapping square tiles a frame is cut into, per axis and then as their Cartesian product in
row-major order.  The tiled-*training* helpers of that module (random origins, augmentation halo, frame-grouped sampler) are not
built here.
"""
from __future__ import annotations

from typing import List, Tuple


def axis_tile_origins(image_dim: int, tile_size: int, overlap: int, output_stride: int, max_stride: int = 1, min_overlap_fraction: float = 0.25) -> List[int]:
    """Ascending, distinct tile origins along one axis, each a multiple of ``output_stride``.

    * an axis no longer than a tile has the single origin 0 (the tile is zero padded);
    * the overlap is raised to ``round(min_overlap_fraction * tile_size)``, the step ``tile_size - overlap`` is rounded down to a
      multiple of ``max_stride`` (when the step reaches it and ``output_stride`` divides it) or else of ``output_stride``, and
      never falls below ``output_stride``;
    * origins advance by the step while a tile ends strictly inside the axis; the last tile is pushed inwards to end at the far
      edge (rounded down to the ``output_stride`` grid) and dropped when it repeats the one before.
    """
    if image_dim <= tile_size:
        return [0]
    step = tile_size - max(overlap, round(min_overlap_fraction * tile_size))
    unit = max_stride if (step >= max_stride and max_stride % output_stride == 0) else output_stride
    step = max(step // unit * unit, output_stride)
    origins = [pos // output_stride * output_stride for pos in range(0, image_dim - tile_size, step)]
    last = (image_dim - tile_size) // output_stride * output_stride
    if not origins or origins[-1] != last:
        origins.append(last)
    return origins


def generate_tile_grid(image_hw: Tuple[int, int], tile_size: int, overlap: int, output_stride: int, max_stride: int = 1,
                       min_overlap_fraction: float = 0.25) -> List[Tuple[int, int]]:
    """``(y0, x0)`` top-left tile origins in input pixels covering an ``(H, W)`` frame, row-major (every x origin of the first y
    origin, then of the next); never empty.  See ``axis_tile_origins`` for the snapping rules."""
    ys = axis_tile_origins(image_hw[0], tile_size, overlap, output_stride, max_stride, min_overlap_fraction)
    xs = axis_tile_origins(image_hw[1], tile_size, overlap, output_stride, max_stride, min_overlap_fraction)
    return [(y0, x0) for y0 in ys for x0 in xs]
