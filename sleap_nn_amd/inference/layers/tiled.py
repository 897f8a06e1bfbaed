"""``TiledLayer``: sliding-window inference around a single-instance layer (``sleap_nn/inference/layers/tiled.py:135-350``).

A frame much larger than the model's training tiles is preprocessed at native resolution (channel coercion, ``input_scale``,
pad to ``output_stride``; no sizematcher), cut into overlapping square tiles on the ``output_stride`` grid, forwarded in batches
of at most ``tile_batch_size`` tiles, and the per-tile confidence maps are stitched into one map per frame with an importance
window; one global peak per node is then read from the stitched map.  The tile offset is in the paste position, so there is
no ``add_crop_offset``.  Like ``TopDownLayer`` this is not an ``InferenceLayer`` subclass.

The two memory-bound steps are one launch each for the whole batch: ``ph_tile_extract`` (all tiles of all frames) and
``ph_tile_merge`` (the stitch as a gather over a tile-map arena, bit-identical to the reference's ACC / CNT canvas; DESIGN.md
section 10).
"""
from __future__ import annotations

from typing import Any, Mapping, Optional, Tuple

import torch

from sleap_nn_amd.data.tiling import axis_tile_origins
from sleap_nn_amd.inference.layers.base import ImageInput, InferenceLayer
from sleap_nn_amd.inference.ops.coord import undo_eff_scale, undo_input_scale, undo_stride
from sleap_nn_amd.inference.ops.peaks import find_global_peaks
from sleap_nn_amd.inference.outputs import Outputs
from sleap_nn_amd.inference.preprocess_info import PreprocInfo
from sleap_nn_amd.inference.tile_merger import BLEND_MODES, TileMerger, build_importance_window, extract_tiles, merge_tiles

ACCUMULATOR_DEVICES = ("auto", "cpu", "cuda")

# ``TilingConfig`` defaults of the reference (config/data_config.py:118-134) for the keys inference reads
TILING_DEFAULTS = {"min_overlap_fraction": 0.25, "blend": "gaussian", "sigma_scale": 0.125, "tile_batch_size": None, "accumulator_device": "auto", "cpu_thresh": 0.40}


def tiling_block(preprocessing: Optional[Mapping]) -> Optional[Mapping]:
    """The ``tiling`` mapping of a run directory's ``data_config.preprocessing`` when it is enabled, else ``None``."""
    t = (preprocessing or {}).get("tiling")
    return t if isinstance(t, Mapping) and bool(t.get("enabled")) else None


def tiling_kwargs(preprocessing: Optional[Mapping], tile_size: Optional[int] = None, overlap: Optional[int] = None) -> Optional[dict]:
    """``TiledLayer`` keyword arguments from ``data_config.preprocessing`` (needs no device): ``None`` when tiling is absent or
    disabled; otherwise ``tile_size`` / ``overlap`` as trained (integers are required) and the other keys filled with the
    ``TilingConfig`` defaults, ``tile_batch_size or 8``.  ``tile_size`` / ``overlap`` given here are inference-time overrides that
    are checked, not applied: the geometry is fixed at training time, a different value raises (``check_tiling_parity``,
    config/utils.py:270-309)."""
    t = tiling_block(preprocessing)
    if t is None:
        return None
    for key in ("tile_size", "overlap"):
        v = t.get(key)
        if isinstance(v, bool) or not isinstance(v, int):
            raise ValueError(f"data_config.preprocessing.tiling.enabled is true but tiling.{key}={v!r} is not an integer "
                             "(training writes the tile geometry back into training_config.yaml)")
    for key, given in (("tile_size", tile_size), ("overlap", overlap)):
        if given is not None and int(given) != t[key]:
            raise ValueError(f"{key} override ({given}) does not match the trained tiling geometry ({key}={t[key]}); tiling geometry is "
                             "fixed at train time, retrain to change it")
    kw = {k: (t[k] if t.get(k) is not None else d) for k, d in TILING_DEFAULTS.items()}
    kw["tile_batch_size"] = int(kw["tile_batch_size"] or 8)
    return {"tile_size": int(t["tile_size"]), "overlap": int(t["overlap"]), **kw}


class TiledLayer:
    """``inner_layer``: a built ``SingleInstanceLayer``; its backend, strides, configs and ``_extract_confmaps`` are reused.

    ``tile_size``: square tile side in pixels, a positive multiple of the inner layer's ``max_stride`` and ``output_stride``;
    ``overlap``: requested overlap in pixels (raised to ``min_overlap_fraction * tile_size``); ``blend`` / ``sigma_scale``: the
    importance window; ``tile_batch_size``: the most tiles one backend call gets (chunks run over frame boundaries).

    ``accumulator_device``: ``"cuda"`` stitches with ``ph_tile_merge`` on the backend's device; ``"cpu"`` copies the tile maps to
    the host and runs the torch ``TileMerger`` tile by tile, as the reference does.  ``"auto"`` is ``"cuda"`` here: the
    reference's rule moves its ACC / CNT canvas to the host when it would take more than ``cpu_thresh`` of the free device
    memory, but the gather has no such canvas -- what it holds is the tile-map arena, which the backend's outputs fill on the
    device in any case.  ``cpu_thresh`` is kept for config compatibility and not used.
    """

    def __init__(self, inner_layer: InferenceLayer, tile_size: int, overlap: int, *, blend: str = "gaussian", sigma_scale: float = 0.125,
                 min_overlap_fraction: float = 0.25, tile_batch_size: int = 8, accumulator_device: str = "auto", cpu_thresh: float = 0.40) -> None:
        self.inner = inner_layer
        self.tile_size = int(tile_size)
        self.overlap = int(overlap)
        self.output_stride = int(inner_layer.output_stride)
        self.max_stride = int(inner_layer.max_stride)
        if self.tile_size <= 0 or self.tile_size % self.max_stride or self.tile_size % self.output_stride:
            raise ValueError(f"tile_size={tile_size} must be a positive multiple of max_stride={self.max_stride} and output_stride={self.output_stride}")
        if blend not in BLEND_MODES:
            raise ValueError(f"Unknown importance window mode: {blend!r}. Expected one of {', '.join(repr(m) for m in BLEND_MODES)}.")
        if accumulator_device not in ACCUMULATOR_DEVICES:
            raise ValueError(f"accumulator_device={accumulator_device!r} must be one of {ACCUMULATOR_DEVICES}")
        if int(tile_batch_size) < 1:
            raise ValueError(f"tile_batch_size={tile_batch_size} must be at least 1")
        if inner_layer.backend.does_baked_postproc:
            raise NotImplementedError("Tiled inference is not supported for backends with a baked post-process (exported models)")
        self.backend = inner_layer.backend
        self.tile_batch_size = int(tile_batch_size)
        self.accumulator_device = accumulator_device
        self.cpu_thresh = cpu_thresh
        self._blend = blend
        self._sigma_scale = sigma_scale
        self._min_overlap_fraction = min_overlap_fraction
        self._window_cache: dict = {}  # (th, tw) -> (host window, device window)
        self._grid_cache: dict = {}  # (Hs, Ws) -> per-axis origins (lists, int32 device tensors in input and output pixels)

    # the inner layer's configs, where callers (``Predictor``) read them off the top-level layer
    @property
    def preprocess_config(self):
        return self.inner.preprocess_config

    @property
    def postprocess_config(self):
        return self.inner.postprocess_config

    def _device(self) -> torch.device:
        return torch.device(self.inner.backend.device)

    def _get_window(self, tile_hw: Tuple[int, int]):
        key = (int(tile_hw[0]), int(tile_hw[1]))
        win = self._window_cache.get(key)
        if win is None:
            host = build_importance_window(key, mode=self._blend, sigma_scale=self._sigma_scale)
            win = self._window_cache[key] = (host, host.to(self._device()))
        return win

    def _grid(self, hw: Tuple[int, int]):
        g = self._grid_cache.get(hw)
        if g is None:
            s, dev = self.output_stride, self._device()
            ys, xs = (axis_tile_origins(d, self.tile_size, self.overlap, s, self.max_stride, self._min_overlap_fraction) for d in hw)
            as_dev = lambda v: torch.tensor(v, dtype=torch.int32).to(dev)
            g = self._grid_cache[hw] = (ys, xs, as_dev(ys), as_dev(xs), as_dev([y // s for y in ys]), as_dev([x // s for x in xs]))
        return g

    def tile_origins(self, hw: Tuple[int, int]):
        """``generate_tile_grid`` of a preprocessed ``(Hs, Ws)`` frame with this layer's geometry: ``(y0, x0)`` per tile, row-major."""
        ys, xs = self._grid((int(hw[0]), int(hw[1])))[:2]
        return [(y0, x0) for y0 in ys for x0 in xs]

    def predict(self, image: ImageInput) -> Outputs:
        inner, stride, ts = self.inner, self.output_stride, self.tile_size
        dev = self._device()
        x = InferenceLayer._to_4d_tensor(image).to(dev, non_blocking=True)
        scaled, eff_scale, orig_hw = inner._apply_full_preprocess(x, max_stride=stride, unsqueeze_n_samples=False, skip_sizematcher=True)
        if scaled.dtype not in (torch.uint8, torch.float32):
            scaled = scaled.float()
        input_scale = inner.preprocess_config.scale
        F, _c, Hs, Ws = scaled.shape
        ys, xs, ys_dev, xs_dev, ys_out, xs_out = self._grid((int(Hs), int(Ws)))
        T = len(ys) * len(xs)
        th = tw = ts // stride
        win_host, win_dev = self._get_window((th, tw))
        h, w = Hs // stride, Ws // stride

        tiles = extract_tiles(scaled, ys_dev, xs_dev, ts)  # (F * T, C, ts, ts): the frames of a batch share a size, so one grid and one launch
        arena = None  # (F * T, N, th, tw): every chunk's maps, copied out before the backend's next call reuses its output buffer (same stream)
        for i in range(0, F * T, self.tile_batch_size):
            chunk = tiles[i : i + self.tile_batch_size]
            with torch.inference_mode():
                raw = inner.backend(chunk.unsqueeze(1))
            cms = inner._extract_confmaps(raw).detach()
            if tuple(cms.shape[-2:]) != (th, tw) or cms.shape[0] != chunk.shape[0]:
                raise RuntimeError(f"backend returned confidence maps {tuple(cms.shape)} for {chunk.shape[0]} tiles of {ts} px at output stride {stride}")
            if arena is None:
                arena = torch.empty((F * T, int(cms.shape[1]), th, tw), dtype=torch.float32, device=dev)
            arena[i : i + chunk.shape[0]].copy_(cms, non_blocking=True)

        if self.accumulator_device == "cpu":
            stitched = self._merge_on_host(arena, win_host, ys, xs, F, (Hs, Ws)).to(dev)
        else:
            stitched = merge_tiles(arena, win_dev, ys_out, xs_out, (h, w), frames=F)  # (F, N, h, w)
        pc = inner.postprocess_config
        peaks, vals = find_global_peaks(stitched, threshold=pc.peak_threshold, refinement=pc.effective_refinement, integral_patch_size=pc.integral_patch_size)
        peaks = undo_stride(peaks, stride)
        peaks = undo_input_scale(peaks, input_scale)
        peaks = undo_eff_scale(peaks, eff_scale)
        info = PreprocInfo(original_size=orig_hw, processed_size=(int(Hs), int(Ws)), eff_scale=eff_scale, input_scale=input_scale, output_stride=stride)
        out = Outputs(pred_keypoints=peaks.unsqueeze(1), pred_peak_values=vals.unsqueeze(1), preprocess_info=info)
        if pc.return_confmaps:
            out.pred_confmaps = stitched.detach()
        return out

    __call__ = predict

    def _merge_on_host(self, arena: torch.Tensor, window: torch.Tensor, ys, xs, F: int, proc_hw: Tuple[int, int]) -> torch.Tensor:
        """The reference's stitch (tiled.py:233-263): a canvas of ``max(frame, tile)`` per axis, one ``integrate`` per tile in grid
        order, ``merge()``, crop to the frame's map size."""
        stride, ts = self.output_stride, self.tile_size
        host = arena.cpu()
        T = len(ys) * len(xs)
        canvas = (max(proc_hw[0], ts) // stride, max(proc_hw[1], ts) // stride)
        frames = []
        for f in range(F):
            merger = TileMerger(canvas, int(host.shape[1]), window, device="cpu")
            for t, (y0, x0) in enumerate((y0, x0) for y0 in ys for x0 in xs):
                merger.integrate(host[f * T + t], y0 // stride, x0 // stride)
            frames.append(merger.merge()[:, : proc_hw[0] // stride, : proc_hw[1] // stride])
        return torch.stack(frames)
