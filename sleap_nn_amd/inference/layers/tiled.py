"""``TiledLayer``: sliding-window inference around a single-instance layer (``sleap_nn/inference/layers/tiled.py:135-350``);
``TiledSegmentationLayer`` / ``TiledSemanticSegmentationLayer``: the same around the segmentation layers (``:353-668``), below.

A frame much larger than the model's training tiles is preprocessed at native resolution (channel coercion, ``input_scale``,
pad to ``output_stride``; no sizematcher), cut into overlapping square tiles on the ``output_stride`` grid, forwarded in batches
of at most ``tile_batch_size`` tiles, and the per-tile confidence maps are stitched into one map per frame with an importance
window; one global peak per node is then read from the stitched map.  The tile offset is in the paste position, so there is
no ``add_crop_offset``.  Like ``TopDownLayer`` this is not an ``InferenceLayer`` subclass.

The two memory-bound steps are one launch each for the whole batch: ``ph_tile_extract`` (all tiles of all frames) and
``ph_tile_merge`` (the stitch as a gather over a tile-map arena, bit-identical to the reference's ACC / CNT canvas; DESIGN.md
section 10).  The segmentation wrappers stitch all their heads with one ``ph_tile_merge_heads`` launch (section 10a).
"""
from __future__ import annotations

from typing import Any, List, Mapping, Optional, Tuple

import torch

from sleap_nn_amd.data.tiling import axis_tile_origins
from sleap_nn_amd.inference.layers.base import ImageInput, InferenceLayer
from sleap_nn_amd.inference.ops.coord import undo_eff_scale, undo_input_scale, undo_stride
from sleap_nn_amd.inference.ops.peaks import find_global_peaks
from sleap_nn_amd.inference.outputs import Outputs
from sleap_nn_amd.inference.preprocess_info import PreprocInfo
from sleap_nn_amd.inference.tile_merger import BLEND_MODES, TileMerger, build_importance_window, extract_tiles, merge_tile_heads, merge_tiles

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


class _TiledBase:
    """What the tiled wrappers share: the constructor and its validation, the window and grid caches, the host stitch.

    ``inner_layer``: a built inner layer; its backend, strides and configs are reused.

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


class TiledLayer(_TiledBase):
    """``inner_layer``: a built ``SingleInstanceLayer``; its backend, strides, configs and ``_extract_confmaps`` are reused (constructor: ``_TiledBase``)."""

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


def _extract_tiles_host(frames: torch.Tensor, ys, xs, ts: int) -> torch.Tensor:
    """``extract_tiles`` with torch slicing (``_extract_square_tile`` per tile): ``(F * ny * nx, C, ts, ts)``, zeros past the bottom / right edge."""
    F, C, H, W = frames.shape
    out = frames.new_zeros((F, len(ys) * len(xs), C, ts, ts))
    for t, (y0, x0) in enumerate((y0, x0) for y0 in ys for x0 in xs):
        src = frames[:, :, y0 : y0 + ts, x0 : x0 + ts]
        out[:, t, :, : src.shape[-2], : src.shape[-1]] = src
    return out.reshape(F * len(ys) * len(xs), C, ts, ts)


class TiledSegmentationLayer(_TiledBase):
    """Sliding-window inference around a bottom-up segmentation layer (``sleap_nn/inference/layers/tiled.py:353-553``).

    ``inner_layer``: a built ``SegmentationLayer`` (or its ``CleanupSegmentationLayer`` / ``MergeSegmentationLayer`` subclass); its backend, strides, configs and
    ``postprocess`` are reused verbatim.  The other arguments are ``TiledLayer``'s.  The tiles' foreground (1 channel), centre (1) and offset (2) maps are
    stitched with the same importance window -- probabilities average in the overlaps, and the offset is a displacement, so it averages too -- and the
    stitched heads of the WHOLE batch go through one ``inner.postprocess`` call (the reference stitches and groups frame by frame; the grouping is per frame,
    so the entries are the same).

    On the device the stitch is ONE ``ph_tile_merge_heads`` launch that writes the three contiguous maps the grouping wants.  ``accumulator_device="cpu"``
    is the reference's route: one 4-channel ``TileMerger`` canvas per frame on the host, bit-identical to the kernel, the heads moved back to the backend's
    device.  A backend on the CPU (stub backends) runs extract and stitch with torch slicing and ``TileMerger``, and the host grouping: no GPU is needed.
    ``keep_label_map`` of the inner layer passes through ``postprocess`` as from the plain layer."""

    def __init__(self, inner_layer: InferenceLayer, tile_size: int, overlap: int, *, blend: str = "gaussian", sigma_scale: float = 0.125,
                 min_overlap_fraction: float = 0.25, tile_batch_size: int = 8, accumulator_device: str = "auto", cpu_thresh: float = 0.40) -> None:
        self._check_inner(inner_layer)
        super().__init__(inner_layer, tile_size, overlap, blend=blend, sigma_scale=sigma_scale, min_overlap_fraction=min_overlap_fraction,
                         tile_batch_size=tile_batch_size, accumulator_device=accumulator_device, cpu_thresh=cpu_thresh)

    @staticmethod
    def _check_inner(inner_layer) -> None:
        from sleap_nn_amd.inference.layers.segmentation import SegmentationLayer, SemanticSegmentationLayer

        if not isinstance(inner_layer, SegmentationLayer) or isinstance(inner_layer, SemanticSegmentationLayer):
            raise TypeError(f"TiledSegmentationLayer wraps a SegmentationLayer (or its cleanup / merge subclass), got {type(inner_layer).__name__}")

    def _head_keys(self) -> Tuple[str, ...]:
        return (self.inner._SEG_KEY, self.inner._CENTER_KEY, self.inner._OFFSET_KEY)

    # the mask-packaging knobs, where callers read them off the top-level layer
    @property
    def mask_output(self):
        return getattr(self.inner, "mask_output", "mask")

    @property
    def polygon_epsilon(self):
        return getattr(self.inner, "polygon_epsilon", 0.01)

    def _stitch(self, image: ImageInput):
        """Tile, forward, stitch: ``(raw_out, info)`` as ``inner.postprocess`` takes them -- ``raw_out[key]`` is ``(F, c, h, w)`` fp32 contiguous per head."""
        inner, stride, ts = self.inner, self.output_stride, self.tile_size
        dev = self._device()
        on_gpu = dev.type == "cuda"
        x = InferenceLayer._to_4d_tensor(image).to(dev, non_blocking=True)
        scaled, eff_scale, orig_hw = inner._apply_full_preprocess(x, max_stride=stride, unsqueeze_n_samples=False, skip_sizematcher=True)
        if scaled.dtype not in (torch.uint8, torch.float32):
            scaled = scaled.float()
        F, _c, Hs, Ws = scaled.shape
        ys, xs, ys_dev, xs_dev, ys_out, xs_out = self._grid((int(Hs), int(Ws)))
        T = len(ys) * len(xs)
        th = tw = ts // stride
        win_host, win_dev = self._get_window((th, tw))
        h, w = Hs // stride, Ws // stride
        keys = self._head_keys()

        tiles = extract_tiles(scaled, ys_dev, xs_dev, ts) if on_gpu else _extract_tiles_host(scaled, ys, xs, ts)  # (F * T, C, ts, ts)
        arenas: Optional[List[torch.Tensor]] = None  # per head (F * T, c_k, th, tw): copied out before the backend's next call reuses its output buffer (same stream)
        for i in range(0, F * T, self.tile_batch_size):
            chunk = tiles[i : i + self.tile_batch_size]
            with torch.inference_mode():
                raw = inner.backend(chunk.unsqueeze(1))
            maps = [raw[k].detach() for k in keys]
            for k, m in zip(keys, maps):
                if m.dim() != 4 or tuple(m.shape[-2:]) != (th, tw) or m.shape[0] != chunk.shape[0]:
                    raise RuntimeError(f"backend returned {k} maps {tuple(m.shape)} for {chunk.shape[0]} tiles of {ts} px at output stride {stride}")
            if arenas is None:
                arenas = [torch.empty((F * T, int(m.shape[1]), th, tw), dtype=torch.float32, device=dev) for m in maps]
            for a, m in zip(arenas, maps):
                a[i : i + chunk.shape[0]].copy_(m, non_blocking=True)

        if on_gpu and self.accumulator_device != "cpu":
            heads = merge_tile_heads(arenas, win_dev, ys_out, xs_out, (h, w), frames=F)
        else:  # one canvas of all channels per frame, as the reference's
            canvas = self._merge_on_host(torch.cat([a.cpu() for a in arenas], dim=1), win_host, ys, xs, F, (Hs, Ws))
            heads = [part.contiguous().to(dev) for part in torch.split(canvas, [int(a.shape[1]) for a in arenas], dim=1)]
        info = PreprocInfo(original_size=orig_hw, processed_size=(int(Hs), int(Ws)), eff_scale=eff_scale, input_scale=inner.preprocess_config.scale, output_stride=stride)
        return dict(zip(keys, heads)), info

    def predict(self, image: ImageInput) -> Outputs:
        raw_out, info = self._stitch(image)
        return self.inner.postprocess(raw_out, info)  # frame / video indices are the Predictor's to stamp

    __call__ = predict


class TiledSemanticSegmentationLayer(TiledSegmentationLayer):
    """The one-head twin (``sleap_nn/inference/layers/tiled.py:556-668``) around a ``SemanticSegmentationLayer``: only the foreground is stitched
    (``ph_tile_merge_heads`` with K = 1) and thresholded into one mask per frame by the inner ``postprocess``."""

    @staticmethod
    def _check_inner(inner_layer) -> None:
        from sleap_nn_amd.inference.layers.segmentation import SemanticSegmentationLayer

        if not isinstance(inner_layer, SemanticSegmentationLayer):
            raise TypeError(f"TiledSemanticSegmentationLayer wraps a SemanticSegmentationLayer, got {type(inner_layer).__name__}")

    def _head_keys(self) -> Tuple[str, ...]:
        return (self.inner._SEG_KEY,)
