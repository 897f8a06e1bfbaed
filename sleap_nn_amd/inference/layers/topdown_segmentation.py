"""``CenteredInstanceMaskLayer`` / ``TopDownSegmentationLayer`` (sleap_nn/inference/layers/topdown_segmentation.py:40-284): top-down instance
segmentation -- a centroid model finds the animals, a lone ``SegmentationHead`` on each crop predicts one mask per animal.

Stage 1, the sizematched frames and the crop gather are ``TopDownLayer``'s, unchanged (``ph_centroid_select``, ``ph_crop_bboxes``); only the stage-2
emission differs: the crop network's probabilities are thresholded, counted and summed on the device (``ph_seg_semantic`` with one "frame" per crop),
and every crop becomes one ``pred_masks`` entry ``{"mask", "score", "scale", "offset"}`` whose offset / scale (host arithmetic,
``ops.segmentation.crop_mask_geometry``) place it in the frame.  With ``place_masks=True`` the crop masks are also placed into frame space on the device
(``ph_seg_place_crops``): ``Outputs.pred_mask_stack`` uint8 (B, P, H, W) with ``P = max_instances`` and ``Outputs.pred_mask_counts`` int32 (B,), the
form the mask evaluator reads without a host round trip.

Not built (each raises ``NotImplementedError``): ``mask_output`` other than ``"mask"``, the ground-truth-centroid path (a seg run directory alone),
tiled wrappers, and training of this model type.
"""
from __future__ import annotations

import ctypes as C
from typing import List, Optional, Tuple

import numpy as np
import torch

from sleap_nn_amd.inference.backends import ModelBackend
from sleap_nn_amd.inference.layers.base import InferenceLayer
from sleap_nn_amd.inference.layers.centroid import CentroidLayer
from sleap_nn_amd.inference.layers.configs import PostprocessConfig, PreprocessConfig
from sleap_nn_amd.inference.layers.segmentation import _refuse
from sleap_nn_amd.inference.layers.topdown import TopDownLayer
from sleap_nn_amd.inference.ops.crops import make_centered_bboxes
from sleap_nn_amd.inference.ops.segmentation import crop_mask_geometry, place_crop_masks, semantic_enqueue, semantic_finish
from sleap_nn_amd.inference.outputs import Outputs
from sleap_nn_amd.inference.preprocess_info import PreprocInfo

MAX_PLACED_MASKS = 64  # ph_seg_place_crops / ph_mask_pair_stats: masks per frame of a device stack


class CenteredInstanceMaskLayer(InferenceLayer):
    """One foreground mask per crop (topdown_segmentation.py:40-114).  The backend's ``"SegmentationHead"`` holds probabilities (the sigmoid is the head
    op's epilogue here).  ``postprocess`` returns ``Outputs(crops=masks uint8 (N, 1, h, w), instance_scores=(N, 1) float32)``: the score is the mean
    probability over the mask, 0 for an empty one.  GPU tensors: the masks stay on the device, the per-crop counts and sums are the only host read."""

    _HEAD_OUTPUT_KEY = "SegmentationHead"

    def __init__(self, backend: ModelBackend, output_stride: int, max_stride: int = 1, fg_threshold: float = 0.5,
                 preprocess_config: Optional[PreprocessConfig] = None, postprocess_config: Optional[PostprocessConfig] = None) -> None:
        super().__init__(backend, preprocess_config or PreprocessConfig(), postprocess_config or PostprocessConfig(), output_stride, max_stride)
        self.fg_threshold = float(fg_threshold)
        self.use_gt_peaks = False  # (read by the composed layer in the reference; a mask layer never takes the ground-truth branch)

    @property
    def warmup_input_shape(self):
        return (1, 1, 64, 64)

    def _masks_enqueue(self, raw_out: dict, host_masks: bool) -> dict:
        """The device stage of ``postprocess`` for GPU tensors: no host synchronisation (``ops.segmentation.semantic_enqueue`` with B = the crops)."""
        return semantic_enqueue(self._extract_confmaps(raw_out), self.fg_threshold, host_masks=host_masks)

    def postprocess(self, raw_out: dict, info: PreprocInfo) -> Outputs:
        probs = self._extract_confmaps(raw_out).detach()
        if probs.is_cuda:
            hd = self._masks_enqueue(raw_out, host_masks=False)
            _m, _counts, scores = semantic_finish(hd)
            return Outputs(crops=hd["mask_dev"].unsqueeze(1), instance_scores=torch.from_numpy(scores.astype(np.float32)).view(-1, 1), preprocess_info=info)
        probs = probs.to(torch.float32)
        masks = (probs > self.fg_threshold).float()
        score = (probs * masks).sum(dim=(2, 3)) / masks.sum(dim=(2, 3)).clamp(min=1.0)
        return Outputs(crops=masks.to(torch.uint8), instance_scores=score, preprocess_info=info)


class TopDownSegmentationLayer(TopDownLayer):
    """Centroids -> crops -> one mask per crop, emitted as ``Outputs(pred_masks=..., preprocess_info=...)`` and nothing else: no centroids, no keypoints
    (topdown_segmentation.py:117-284).  Entries are in ``torch.nonzero`` order of the valid centroids (frame, then slot); ``offset`` is the floored sized
    top-left of the crop divided by the frame's sizematcher scale, ``scale = eff * input_scale / stride``; a batch without a valid centroid gives
    ``[[] for _ in range(B)]``.  ``place_masks=True`` adds ``pred_mask_stack`` / ``pred_mask_counts`` (module docstring); slot j of a frame is its j-th entry."""

    _PIPELINED = False  # Predictor runs this layer batch by batch, like the other segmentation layers (no multi-lane path, no replicas)

    def __init__(self, centroid_layer: CentroidLayer, centered_instance_layer: CenteredInstanceMaskLayer, crop_size: Tuple[int, int], mask_output: str = "mask",
                 polygon_epsilon: float = 0.01, centroid_nms: bool = False, centroid_nms_threshold: float = 0.5, place_masks: bool = False) -> None:
        super().__init__(centroid_layer, centered_instance_layer, crop_size, centroid_nms=centroid_nms, centroid_nms_threshold=centroid_nms_threshold, return_crops=False)
        _refuse(mask_output=(str(mask_output), "mask"))
        self.mask_output = "mask"
        self.polygon_epsilon = float(polygon_epsilon)
        self.place_masks = bool(place_masks)

    def _empty(self, B: int, I: int, frame_hw, dev, info) -> Outputs:
        out = Outputs(pred_masks=[[] for _ in range(B)], preprocess_info=info)
        if self.place_masks:
            out.pred_mask_stack = torch.zeros((B, self._stack_slots(I), int(frame_hw[0]), int(frame_hw[1])), dtype=torch.uint8, device=dev)
            out.pred_mask_counts = torch.zeros(B, dtype=torch.int32)
        return out

    @staticmethod
    def _stack_slots(I: int) -> int:
        if not 1 <= I <= MAX_PLACED_MASKS:
            raise ValueError(f"place_masks=True holds at most {MAX_PLACED_MASKS} masks per frame, this batch has {I} instance slots: set max_instances")
        return I

    def _emit(self, crops: torch.Tensor, topleft_sized: np.ndarray, samples: np.ndarray, pos_of_slot: torch.Tensor, B: int, I: int, frame_hw, info: PreprocInfo) -> Outputs:
        """Stage 2 on gathered crops: the crop network, the masks / counts / sums (device), the geometry (host), the optional placement (device), and one
        wait: for the masks, counts and sums in pinned memory."""
        il = self.centered_instance_layer
        n = int(crops.shape[0])
        x, _crop_info = il.preprocess(crops)
        hd = il._masks_enqueue(il.backend(x), host_masks=True)
        mask_dev = hd["mask_dev"]
        eff = info.eff_scale.detach().cpu().numpy().astype(np.float32)[samples]
        geo = crop_mask_geometry(topleft_sized, eff, float(il.preprocess_config.scale), il.output_stride, self.crop_size, tuple(mask_dev.shape[-2:]))
        stack = None
        if self.place_masks:
            stack = place_crop_masks(mask_dev, pos_of_slot, geo.origin, geo.extent, frame_hw, self._stack_slots(I))
        masks, _counts, scores = semantic_finish(hd)
        pred_masks: List[List[dict]] = [[] for _ in range(B)]
        for k in range(n):
            pred_masks[int(samples[k])].append({"mask": np.ascontiguousarray(masks[k], dtype=bool), "score": float(scores[k]),
                                                "scale": (float(geo.scale[k, 0]), float(geo.scale[k, 1])), "offset": (float(geo.offset[k, 0]), float(geo.offset[k, 1]))})
        out = Outputs(pred_masks=pred_masks, preprocess_info=info)
        if stack is not None:
            out.pred_mask_stack = stack
            out.pred_mask_counts = torch.from_numpy(np.bincount(samples, minlength=B).astype(np.int32))
        return out

    def _gather(self, x: torch.Tensor, topleft: torch.Tensor, samples: torch.Tensor, n: int) -> torch.Tensor:
        """``ph_crop_bboxes`` at the configured crop size (always ``crop_size``, whatever the first box's float32 corners span)."""
        from sleap_nn_amd import _lib as L

        if x.dtype == torch.uint8:
            code = 0
        elif x.dtype == torch.float32:
            code = 1
        else:
            raise TypeError(f"crop_bboxes supports uint8 and float32 images, got {x.dtype}")
        x = x.contiguous()
        B, Cc, H, W = x.shape
        ch, cw = self.crop_size
        crops = torch.empty((n, Cc, ch, cw), dtype=x.dtype, device=x.device)
        with torch.cuda.device(x.device):
            L.check(L.lib().ph_crop_bboxes(C.c_void_p(x.data_ptr()), code, B, Cc, H, W, C.c_void_p(topleft.data_ptr()), C.c_void_p(samples.data_ptr()), n, ch, cw,
                                           C.c_void_p(crops.data_ptr()), L.current_stream_ptr()))
        return crops

    def _finish(self, h: dict) -> Outputs:
        if h["slow"]:
            return self._predict_with_host_nms(h["x"])
        cl = self.centroid_layer
        x = h["x"]
        dev = x.device
        ch, cw = self.crop_size
        frame_hw = tuple(x.shape[-2:])
        sel = cl._select_finish(h["sel"], h["info"], (ch, cw))
        I, n_valid = sel["I"], sel["n_valid"]
        B = int(sel["centroids"].shape[0])
        if n_valid == 0:
            return self._empty(B, I, frame_hw, dev, h["info"])
        crops = self._gather(self._sized_frames(x, h["info"]), sel["list_tl"], sel["list_sample"], n_valid)
        # the crop corners and frames of the list (a few numbers; the selection kernel has already run behind the counts read) for the host geometry
        lists = torch.cat([sel["list_tl"][:n_valid].flatten(), sel["list_sample"][:n_valid].to(torch.float32)]).cpu().numpy()
        topleft, samples = lists[: 2 * n_valid].reshape(n_valid, 2), lists[2 * n_valid :].astype(np.int64)
        return self._emit(crops, topleft, samples, sel["pos_of_slot"], B, I, frame_hw, h["info"])

    def _predict_with_host_nms(self, x: torch.Tensor) -> Outputs:
        """The path with centroid NMS: centroids -> host -> mask -> crops, as ``TopDownLayer`` walks it, then the same stage 2."""
        cout = self.centroid_layer.predict(x)
        centroids, cvals = cout.pred_centroids, cout.pred_centroid_values
        B, I, _ = centroids.shape
        dev = centroids.device
        info = cout.preprocess_info
        frame_hw = tuple(x.shape[-2:])
        valid = ~torch.isnan(centroids).any(dim=-1)
        valid = valid & self._centroid_nms_mask(centroids, cvals, valid)
        idx = valid.nonzero(as_tuple=False)
        n_valid = int(idx.shape[0])
        if n_valid == 0:
            return self._empty(B, I, frame_hw, dev, info)
        ch, cw = self.crop_size
        eff = info.eff_scale.to(dev, torch.float32)
        vc = centroids[idx[:, 0], idx[:, 1]] * eff[idx[:, 0]].view(-1, 1)  # sized space (layers/topdown.py:147)
        bboxes = make_centered_bboxes(vc, ch, cw)
        topleft = bboxes[:, 0, :].to(torch.float32).contiguous()
        crops = self._gather(self._sized_frames(x, info).to(dev), topleft, idx[:, 0].to(torch.int32).contiguous(), n_valid)
        samples = idx[:, 0].cpu().numpy().astype(np.int64)
        # slot j of a frame = its j-th kept centroid (NMS may leave gaps among the centroid slots; the stack has none)
        first = np.searchsorted(samples, np.arange(B))
        pos = np.full(B * I, -1, dtype=np.int32)
        pos[samples * I + (np.arange(n_valid) - first[samples])] = np.arange(n_valid, dtype=np.int32)
        return self._emit(crops, topleft.cpu().numpy(), samples, torch.from_numpy(pos).to(dev), B, I, frame_hw, info)
