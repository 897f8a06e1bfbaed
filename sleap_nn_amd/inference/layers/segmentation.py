"""``SegmentationLayer`` / ``SemanticSegmentationLayer`` (sleap_nn/inference/layers/segmentation.py:33-503): bottom-up instance
segmentation and whole-frame semantic segmentation.

The backend's output dict is the reference's ``forward``: probabilities under ``"SegmentationHead"`` (the sigmoid is the head op's
epilogue here), raw maps under ``"InstanceCenterHead"`` / ``"CenterOffsetHead"``.  ``postprocess`` groups the foreground pixels on the
device (``inference/ops/segmentation.py``: centre peaks, pixel assignment, distance gate; one host read per batch: a label map of one
small integer per pixel and a record of centres / scores / counts) and builds ``Outputs.pred_masks`` from the label map; for CPU
tensors the same contract runs on the host.

``mask_cleanup=True`` is ``layers/segmentation_cleanup.py`` (``CleanupSegmentationLayer``) and ``merge_fragments=True`` (the RAG fragment merge)
``layers/segmentation_merge.py`` (``MergeSegmentationLayer``); this class keeps refusing both knobs.  Not built (each raises ``NotImplementedError``
naming the knob): ``mask_cleanup_radius`` (OpenCV morphology), ``merge_fragments`` together with ``mask_cleanup``, ``mask_output`` other than ``"mask"``
(polygon packaging).  The tiled wrappers are ``layers/tiled.py`` (``TiledSegmentationLayer`` / ``TiledSemanticSegmentationLayer``).  Top-down segmentation (``centered_instance_segmentation``) is ``layers/topdown_segmentation.py``.
"""
from __future__ import annotations

import math
from typing import List, Optional

import numpy as np
import torch
import torch.nn.functional as F

from sleap_nn_amd.inference.backends import ModelBackend
from sleap_nn_amd.inference.layers.base import InferenceLayer
from sleap_nn_amd.inference.layers.configs import PostprocessConfig, PreprocessConfig
from sleap_nn_amd.inference.ops.segmentation import group_instances_from_offsets, semantic_masks
from sleap_nn_amd.inference.outputs import Outputs
from sleap_nn_amd.inference.preprocess_info import PreprocInfo


def _refuse(**knobs) -> None:
    for name, (value, allowed) in knobs.items():
        if value != allowed:
            raise NotImplementedError(f"{name}={value!r} is not built on the MI355X path (only {name}={allowed!r}): see inference/layers/segmentation.py")


class SegmentationLayer(InferenceLayer):
    """Constructor arguments and defaults of layers/segmentation.py:102-152.  ``polygon_epsilon`` is stored only (its feature is refused); the ``merge_*`` knobs are stored for ``MergeSegmentationLayer``.

    ``keep_label_map=True`` (not in the reference; the mask tracker's device path, ``sleap_nn_amd/tracking``): ``postprocess`` also returns ``Outputs.pred_label_map``
    (the device label map as ``ph_seg_assign`` / ``ph_seg_gate`` wrote it), ``Outputs.pred_mask_labels`` (per frame the label of each ``pred_masks`` entry; entries
    dropped by the area floor have no slot) and ``Outputs.pred_label_weights`` (per frame the image rows / columns each cell row / column stands for).  Only where
    the label map carries membership: the cleanup / merge subclasses and CPU tensors leave the three fields unset."""

    _KEEPS_LABEL_MAP = True  # the label map of the grouping IS the masks' membership (not after mask cleanup or the fragment merge)
    _SEG_KEY = "SegmentationHead"
    _CENTER_KEY = "InstanceCenterHead"
    _OFFSET_KEY = "CenterOffsetHead"

    def __init__(self, backend: ModelBackend, output_stride: int, max_stride: int = 1, fg_threshold: float = 0.5, min_mask_area: int = 0,
                 max_instances: Optional[int] = None, center_nms_kernel: int = 3, mask_cleanup: bool = False, mask_cleanup_radius: int = 0,
                 distance_gate_alpha: Optional[float] = None, merge_fragments: bool = False, merge_method: str = "greedy",
                 merge_thresholds: tuple = (0.85, 0.6, 0.4), merge_w_valley: float = 1.0, merge_w_offset: float = 0.25, merge_dilate: int = 1,
                 full_res_masks: bool = False, mask_output: str = "mask", polygon_epsilon: float = 0.01,
                 preprocess_config: Optional[PreprocessConfig] = None, postprocess_config: Optional[PostprocessConfig] = None, keep_label_map: bool = False) -> None:
        super().__init__(backend, preprocess_config or PreprocessConfig(), postprocess_config or PostprocessConfig(peak_threshold=0.2), output_stride, max_stride)
        self.keep_label_map = bool(keep_label_map)
        self._axis_cache: dict = {}
        _refuse(mask_cleanup=(bool(mask_cleanup), False), mask_cleanup_radius=(int(mask_cleanup_radius) if int(mask_cleanup_radius) > 0 else 0, 0),
                merge_fragments=(bool(merge_fragments), False), mask_output=(str(mask_output), "mask"))
        self.fg_threshold = fg_threshold
        self.min_mask_area = int(min_mask_area)
        self.max_instances = max_instances
        self.center_nms_kernel = int(center_nms_kernel)
        self.mask_cleanup = False
        self.mask_cleanup_radius = 0
        self.distance_gate_alpha = None if distance_gate_alpha is None else float(distance_gate_alpha)
        self.distance_gate_iters = 3
        self.merge_fragments = False
        self.merge_method = str(merge_method)
        self.merge_thresholds = tuple(merge_thresholds)
        self.merge_w_valley = float(merge_w_valley)
        self.merge_w_offset = float(merge_w_offset)
        self.merge_dilate = int(merge_dilate)
        self.full_res_masks = bool(full_res_masks)
        self.mask_output = "mask"
        self.polygon_epsilon = float(polygon_epsilon)

    @property
    def warmup_input_shape(self):
        return (1, 1, 64, 64)

    # -- geometry (pure host arithmetic on one mask) ------------------------------------------------------------------
    def _mask_to_stride(self, mask: np.ndarray, info: PreprocInfo, b: int) -> tuple:
        """Crop an output-stride mask to its valid (non-pad) extent: ``ceil(round(orig * s) / stride)`` cells clipped to the map, scale ``valid / orig``;
        without metadata the whole map and ``1 / stride`` (layers/segmentation.py:268-325)."""
        orig_h, orig_w = info.original_size
        stride = float(info.output_stride)
        if orig_h == 0 or orig_w == 0:
            return np.ascontiguousarray(mask, dtype=bool), (1.0 / stride, 1.0 / stride), (0.0, 0.0)
        s = self._eff(info, b) * float(info.input_scale)
        scaled_h, scaled_w = max(1, int(round(orig_h * s))), max(1, int(round(orig_w * s)))
        valid_h = min(mask.shape[0], max(1, math.ceil(scaled_h / stride)))
        valid_w = min(mask.shape[1], max(1, math.ceil(scaled_w / stride)))
        return np.ascontiguousarray(mask[:valid_h, :valid_w], dtype=bool), (valid_w / float(orig_w), valid_h / float(orig_h)), (0.0, 0.0)

    def _mask_to_original(self, mask: np.ndarray, info: PreprocInfo, b: int) -> np.ndarray:
        """Output-stride mask -> original resolution: nearest upsample to the processed size, crop the bottom / right pad, nearest resize back
        (layers/segmentation.py:327-364)."""
        return self._map_to_original(mask, info, b).numpy() > 0.5

    def _map_to_original(self, mask: np.ndarray, info: PreprocInfo, b: int) -> torch.Tensor:
        """The resample of ``_mask_to_original`` on any (h, w) map of small numbers, as float32 (nearest: the values come through unchanged)."""
        proc_h, proc_w = info.processed_size
        orig_h, orig_w = info.original_size
        if proc_h == 0 or proc_w == 0:
            proc_h, proc_w = mask.shape[0] * info.output_stride, mask.shape[1] * info.output_stride
        if orig_h == 0 or orig_w == 0:
            orig_h, orig_w = proc_h, proc_w
        t = torch.from_numpy(np.ascontiguousarray(mask)).float()[None, None]
        if tuple(t.shape[-2:]) != (proc_h, proc_w):
            t = F.interpolate(t, size=(proc_h, proc_w), mode="nearest")
        s = self._eff(info, b) * float(info.input_scale)
        scaled_h, scaled_w = min(proc_h, max(1, int(round(orig_h * s)))), min(proc_w, max(1, int(round(orig_w * s))))
        t = t[:, :, :scaled_h, :scaled_w]
        if (scaled_h, scaled_w) != (orig_h, orig_w):
            t = F.interpolate(t, size=(orig_h, orig_w), mode="nearest")
        return t[0, 0]

    def axis_index_maps(self, info: PreprocInfo, b: int, map_hw) -> tuple:
        """``(row_index, col_index)``: the label-map row each IMAGE row reads, and the column each image column reads, when a ``pred_masks`` entry of this layer
        is decoded to the image grid (``decode_mask_to_image_res``).  The resample is separable.  Stride-resolution entries: the integer rule
        ``(Y * valid_h) // He`` over the extent ``He = round(valid_h / sy)`` (``place_crop_masks``); ``full_res_masks``: the composition in ``_mask_to_original``,
        run on an index map.  Cached per geometry."""
        h, w = int(map_hw[0]), int(map_hw[1])
        key = (h, w, tuple(info.original_size), tuple(info.processed_size), self._eff(info, b), float(info.input_scale), int(info.output_stride), self.full_res_masks)
        hit = self._axis_cache.get(key)
        if hit is not None:
            return hit
        if self.full_res_masks:
            rows = self._map_to_original(np.broadcast_to(np.arange(h, dtype=np.float32)[:, None], (h, w)), info, b)[:, 0].numpy().astype(np.int64)
            cols = self._map_to_original(np.broadcast_to(np.arange(w, dtype=np.float32)[None, :], (h, w)), info, b)[0, :].numpy().astype(np.int64)
        else:
            m, scale, _off = self._mask_to_stride(np.zeros((h, w), dtype=bool), info, b)
            He, We = int(round(m.shape[0] / scale[1])), int(round(m.shape[1] / scale[0]))
            rows = (np.arange(He, dtype=np.int64) * m.shape[0]) // max(He, 1)
            cols = (np.arange(We, dtype=np.int64) * m.shape[1]) // max(We, 1)
        if len(self._axis_cache) >= 16:
            self._axis_cache.clear()
        self._axis_cache[key] = (rows, cols)
        return rows, cols

    @staticmethod
    def _eff(info: PreprocInfo, b: int) -> float:
        return float(info.eff_scale[b]) if info.eff_scale is not None and info.eff_scale.numel() > b else 1.0

    def _package(self, mask: np.ndarray, score: float, info: PreprocInfo, b: int) -> Optional[dict]:
        """One ``pred_masks`` entry, or None when the mask is below the area floor (layers/segmentation.py:228-263): the floor ``max(1, min_mask_area)`` is in
        original pixels, ``max(1, ceil(floor sx sy))`` in stride cells, compared with the cropped mask's sum."""
        floor = max(1, self.min_mask_area)
        if self.full_res_masks:
            out, scale, offset = self._mask_to_original(mask, info, b), (1.0, 1.0), (0.0, 0.0)
        else:
            out, scale, offset = self._mask_to_stride(mask, info, b)
            floor = max(1, math.ceil(floor * scale[0] * scale[1]))
        if int(out.sum()) < floor:
            return None
        return {"mask": out, "score": float(score), "scale": scale, "offset": offset}

    def _grouping_kw(self) -> dict:
        """Further keywords of the grouping (the fragment merge's, in ``MergeSegmentationLayer``)."""
        return {}

    def postprocess(self, raw_out: dict, info: PreprocInfo) -> Outputs:
        pc = self.postprocess_config
        max_instances = getattr(pc, "max_instances", None)
        if max_instances is None:
            max_instances = self.max_instances
        g = group_instances_from_offsets(raw_out[self._SEG_KEY], raw_out[self._CENTER_KEY], raw_out[self._OFFSET_KEY], fg_threshold=self.fg_threshold,
                                         peak_threshold=pc.peak_threshold, output_stride=self.output_stride, max_instances=max_instances,
                                         center_nms_kernel=self.center_nms_kernel, distance_gate_alpha=self.distance_gate_alpha,
                                         distance_gate_iters=self.distance_gate_iters, mask_cleanup=self.mask_cleanup, **self._grouping_kw())
        pred_masks: List[List[dict]] = []
        kept: List[List[int]] = []
        for b in range(g.labels.shape[0]):
            frame = [self._package(inst["mask"], inst["score"], info, b) for inst in g.instances(b, self.output_stride)]
            pred_masks.append([m for m in frame if m is not None])
            kept.append([int(k) for k, m in zip(np.nonzero(g.counts[b] > 0)[0], frame) if m is not None])  # (``Grouping.instances`` walks the same labels in this order)
        if self.keep_label_map and self._KEEPS_LABEL_MAP and g.labels_dev is not None:
            from sleap_nn_amd.tracking.scoring import axis_weights

            h, w = g.labels.shape[1:]
            weights = [axis_weights(*self.axis_index_maps(info, b, (h, w)), h, w) for b in range(g.labels.shape[0])]
            return Outputs(pred_masks=pred_masks, preprocess_info=info, pred_label_map=g.labels_dev, pred_mask_labels=kept, pred_label_weights=weights)
        return Outputs(pred_masks=pred_masks, preprocess_info=info)


class SemanticSegmentationLayer(SegmentationLayer):
    """One whole-frame foreground mask per frame, score = mean probability over it (layers/segmentation.py:367-503)."""

    def __init__(self, backend: ModelBackend, output_stride: int, max_stride: int = 1, fg_threshold: float = 0.5, min_mask_area: int = 0, full_res_masks: bool = False,
                 mask_output: str = "mask", polygon_epsilon: float = 0.01, preprocess_config: Optional[PreprocessConfig] = None,
                 postprocess_config: Optional[PostprocessConfig] = None) -> None:
        super().__init__(backend, output_stride, max_stride=max_stride, fg_threshold=fg_threshold, min_mask_area=min_mask_area, full_res_masks=full_res_masks,
                         mask_output=mask_output, polygon_epsilon=polygon_epsilon, preprocess_config=preprocess_config, postprocess_config=postprocess_config)

    def postprocess(self, raw_out: dict, info: PreprocInfo) -> Outputs:
        masks, counts, scores = semantic_masks(raw_out[self._SEG_KEY], self.fg_threshold)
        pred_masks: List[List[dict]] = []
        for b in range(masks.shape[0]):
            m = self._package(masks[b], scores[b], info, b) if counts[b] > 0 else None
            pred_masks.append([m] if m is not None else [])
        return Outputs(pred_masks=pred_masks, preprocess_info=info)
