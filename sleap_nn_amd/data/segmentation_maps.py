"""Training targets of the segmentation model types from instance masks, for whole batches.

``generate_foreground_mask``, ``generate_center_heatmap``, ``generate_center_offsets`` and ``compute_mask_centroids`` keep the
reference's names and defaults (``sleap_nn/data/segmentation_maps.py``) but take ``masks`` as one ``(B, I, H, W)`` uint8 / bool
tensor (non-zero = foreground, of the image's size) and ``n_instances`` ``(B,)``: slots at or beyond ``n_instances[b]`` are
padding and are ignored, which is different from a real, empty mask (image-centre centroid, and a Gaussian in the centre map).
They dispatch on the tensor's device, as ``data/targets.py`` does: masks on the GPU take ``ph_render_seg_targets``, CPU masks a
torch form of the same contract, which the CPU tests pin against the reference's recorded results.

What is computed: output grids are ``(H // s, W // s)``; a cell's window is that of
``adaptive_avg_pool2d`` (``F.interpolate(mode="area")``), ``[floor(i H / out), ceil((i + 1) H / out))``; "area average > 0.5" is
decided on integers (``2 count > window``).  Among the instances that cover a cell the one with the smallest full-resolution area
wins the offsets, the higher index among equal areas -- what the reference's stable descending sort followed by in-order
overwriting leaves.  The masks of a frame that differ in size from the image, which the reference crops, are not handled.

``SegmentationTargetGenerator`` turns a batch's masks into the dict ``SegmentationTrainingModule.training_step`` takes.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Dict, Optional, Tuple

import torch

from sleap_nn_amd import _lib as L

SEGMENTATION_TARGET_TYPES = ("bottomup_segmentation", "semantic_segmentation")


def _prep(masks: torch.Tensor, n_instances, img_hw=None) -> Tuple[torch.Tensor, torch.Tensor]:
    if masks.dim() != 4:
        raise ValueError(f"masks must be (B, I, H, W), got {tuple(masks.shape)}")
    B, I, H, W = masks.shape
    if img_hw is not None and (int(img_hw[0]), int(img_hw[1])) != (H, W):
        raise ValueError(f"masks of size {(H, W)} for an image of size {tuple(img_hw)}: masks must have the image's size")
    m = masks if masks.dtype == torch.uint8 else (masks != 0).to(torch.uint8)
    if n_instances is None:
        n = torch.full((B,), I, dtype=torch.int32, device=m.device)
    else:
        n = torch.as_tensor(n_instances).to(m.device, torch.int32).reshape(-1)
        if n.numel() != B:
            raise ValueError(f"n_instances has {n.numel()} entries for a batch of {B}")
    return m.contiguous(), n.contiguous()


def _grid_hw(H: int, W: int, stride: int) -> Tuple[int, int]:
    stride = int(stride)
    if stride < 1 or H // stride < 1 or W // stride < 1:
        raise ValueError(f"output_stride {stride} does not fit masks of size {(H, W)}")
    return H // stride, W // stride


def _valid(n: torch.Tensor, I: int) -> torch.Tensor:
    return torch.arange(I, device=n.device).view(1, I) < n.view(-1, 1).clamp(0, I)  # (B, I)


# ---- torch form (either device; the CPU tests pin it) -------------------------------------------------------------------------------


def _stats_torch(m: torch.Tensor, n: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    B, I, H, W = m.shape
    nz = (m != 0).to(torch.int64)
    area = nz.sum(dim=(2, 3))
    sx = (nz.sum(dim=2) * torch.arange(W, device=m.device)).sum(dim=-1)
    sy = (nz.sum(dim=3) * torch.arange(H, device=m.device)).sum(dim=-1)
    cnt = area.clamp(min=1).to(torch.float64)
    cx = torch.where(area > 0, sx.to(torch.float64) / cnt, torch.full_like(cnt, W / 2.0))
    cy = torch.where(area > 0, sy.to(torch.float64) / cnt, torch.full_like(cnt, H / 2.0))
    cent = torch.stack([cx, cy], dim=-1).to(torch.float32)  # one fp64 division each, rounded to fp32
    valid = _valid(n, I)
    cent = torch.where(valid.unsqueeze(-1), cent, torch.full_like(cent, float("nan")))
    return cent, torch.where(valid, area, torch.zeros_like(area))


def _window_counts(nz: torch.Tensor, h: int, w: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """``nz`` (..., H, W) int64 0/1 -> pixel count per adaptive-pool window (..., h, w), and the window sizes (h, w)."""
    H, W = nz.shape[-2:]
    dev = nz.device
    S = torch.nn.functional.pad(nz.cumsum(-1).cumsum(-2), (1, 0, 1, 0))
    iy, ix = torch.arange(h, device=dev), torch.arange(w, device=dev)
    y0, y1 = (iy * H) // h, ((iy + 1) * H + h - 1) // h
    x0, x1 = (ix * W) // w, ((ix + 1) * W + w - 1) // w
    cnt = S[..., y1[:, None], x1[None, :]] - S[..., y0[:, None], x1[None, :]] - S[..., y1[:, None], x0[None, :]] + S[..., y0[:, None], x0[None, :]]
    return cnt, (y1 - y0)[:, None] * (x1 - x0)[None, :]


def _grid_xy(h: int, w: int, stride: int, device):
    xv = torch.arange(w, dtype=torch.float32, device=device) * stride + stride / 2.0
    yv = torch.arange(h, dtype=torch.float32, device=device) * stride + stride / 2.0
    return xv, yv


def _foreground_torch(m, n, stride, maxpool):
    B, I, H, W = m.shape
    h, w = _grid_hw(H, W, stride)
    union = ((m != 0) & _valid(n, I)[:, :, None, None]).any(dim=1).to(torch.int64)
    cnt, win = _window_counts(union, h, w)
    return ((cnt > 0) if maxpool else (2 * cnt > win)).to(torch.float32).unsqueeze(1)


def _center_torch(m, n, stride, sigma, cent):
    B, I, H, W = m.shape
    h, w = _grid_hw(H, W, stride)
    out = torch.zeros((B, 1, h, w), dtype=torch.float32, device=m.device)
    if I == 0:
        return out
    xv, yv = _grid_xy(h, w, stride, m.device)
    scaled_sigma = float(sigma) * int(stride)
    cx, cy = cent[..., 0, None, None], cent[..., 1, None, None]
    g = torch.exp(-((xv.view(1, 1, 1, -1) - cx) ** 2 + (yv.view(1, 1, -1, 1) - cy) ** 2) / (2 * scaled_sigma**2))
    g = torch.where(_valid(n, I)[:, :, None, None], g, torch.zeros_like(g))
    return g.amax(dim=1, keepdim=True)


def _offsets_torch(m, n, stride, cent, area, out3=None):
    B, I, H, W = m.shape
    h, w = _grid_hw(H, W, stride)
    if out3 is None:
        out3 = torch.empty((B, 3, h, w), dtype=torch.float32, device=m.device)
    out3.zero_()
    if I > 0:
        cnt, win = _window_counts((m != 0).to(torch.int64), h, w)  # (B, I, h, w)
        covers = (2 * cnt > win) & _valid(n, I)[:, :, None, None]
        # smallest area first, then the higher index: one integer key per (instance, cell)
        key = area[:, :, None, None] * I + (I - 1 - torch.arange(I, device=m.device)).view(1, I, 1, 1)
        key = torch.where(covers, key, torch.full_like(key, torch.iinfo(torch.int64).max))
        winner = key.argmin(dim=1)  # (B, h, w)
        any_cover = covers.any(dim=1)
        xv, yv = _grid_xy(h, w, stride, m.device)
        c = torch.nan_to_num(cent)
        cx = torch.gather(c[..., 0], 1, winner.view(B, -1)).view(B, h, w)
        cy = torch.gather(c[..., 1], 1, winner.view(B, -1)).view(B, h, w)
        zero = torch.zeros((), dtype=torch.float32, device=m.device)
        out3[:, 0] = torch.where(any_cover, cx - xv.view(1, 1, -1), zero)
        out3[:, 1] = torch.where(any_cover, cy - yv.view(1, -1, 1), zero)
        out3[:, 2] = any_cover.to(torch.float32)
    return out3[:, :2], out3[:, 2:3]


# ---- device form -------------------------------------------------------------------------------------------------------------------


def _render_device(m, n, stride, sigma, maxpool, cent, area, compute_stats, fg=None, center=None, out3=None):
    B, I, H, W = m.shape
    off_ptr = wt_ptr = None
    bs = 0
    if out3 is not None:
        bs = out3.stride(0)
        off_ptr, wt_ptr = C.c_void_p(out3.data_ptr()), C.c_void_p(out3.data_ptr() + 4 * 2 * out3.shape[2] * out3.shape[3])
    with torch.cuda.device(m.device):
        L.check(L.lib().ph_render_seg_targets(C.c_void_p(m.data_ptr()), C.c_void_p(n.data_ptr()), B, I, H, W, int(stride), float(sigma), 1 if maxpool else 0,
                                              1 if compute_stats else 0, C.c_void_p(cent.data_ptr()), C.c_void_p(area.data_ptr()),
                                              C.c_void_p(fg.data_ptr()) if fg is not None else None, C.c_void_p(center.data_ptr()) if center is not None else None,
                                              off_ptr, bs, wt_ptr, bs, L.current_stream_ptr()))


def _stats(m, n):
    B, I = m.shape[:2]
    if not m.is_cuda or B == 0 or I == 0:
        return _stats_torch(m, n)
    cent = torch.empty((B, I, 2), dtype=torch.float32, device=m.device)
    area = torch.empty((B, I), dtype=torch.int64, device=m.device)
    _render_device(m, n, 1, 1.0, False, cent, area, True)
    return cent, area


def _centers_arg(centers, m):
    c = torch.as_tensor(centers).to(m.device, torch.float32).contiguous()
    if tuple(c.shape) != (m.shape[0], m.shape[1], 2):
        raise ValueError(f"centers must be (B, I, 2) = {(m.shape[0], m.shape[1], 2)}, got {tuple(c.shape)}")
    return c


def _on_device(m) -> bool:
    return m.is_cuda and m.shape[0] > 0 and m.shape[1] > 0


def _check_out3(out3, B, h, w, device):
    if tuple(out3.shape) != (B, 3, h, w) or out3.dtype != torch.float32 or out3.device != device or not out3.is_contiguous():
        raise ValueError(f"out must be a contiguous fp32 {(B, 3, h, w)} tensor on {device}")


# ---- public functions --------------------------------------------------------------------------------------------------------------


def compute_mask_centroids(masks: torch.Tensor, n_instances=None) -> torch.Tensor:
    """-> (B, I, 2) fp32 (x, y): the mean pixel coordinate of each mask (exact integer sums, one fp64 division, rounded to fp32), the image
    centre ``(W / 2, H / 2)`` for a real, empty mask, NaN in padding slots."""
    m, n = _prep(masks, n_instances)
    return _stats(m, n)[0]


def generate_foreground_mask(masks: torch.Tensor, img_hw: Optional[Tuple[int, int]] = None, output_stride: int = 2, maxpool: bool = False, n_instances=None) -> torch.Tensor:
    """-> (B, 1, H // s, W // s) fp32 in {0, 1}: the union of a frame's masks, area-pooled; a cell is foreground when more than half of its window
    is (exactly half is background), with ``maxpool`` when any pixel is."""
    m, n = _prep(masks, n_instances, img_hw)
    B, I, H, W = m.shape
    h, w = _grid_hw(H, W, output_stride)
    if not _on_device(m):
        return _foreground_torch(m, n, int(output_stride), bool(maxpool))
    fg = torch.empty((B, 1, h, w), dtype=torch.float32, device=m.device)
    cent = torch.empty((B, I, 2), dtype=torch.float32, device=m.device)
    area = torch.empty((B, I), dtype=torch.int64, device=m.device)
    _render_device(m, n, output_stride, 1.0, maxpool, cent, area, False, fg=fg)  # (the union needs neither centroids nor areas)
    return fg


def generate_center_heatmap(masks: torch.Tensor, img_hw: Optional[Tuple[int, int]] = None, output_stride: int = 2, sigma: float = 4.0, centers=None,
                            n_instances=None) -> torch.Tensor:
    """-> (B, 1, H // s, W // s): the maximum over a frame's instances of the Gaussian of width ``sigma * output_stride`` around its centroid, on the
    grid ``i * s + s / 2``.  ``centers`` (B, I, 2): centroids computed before (``compute_mask_centroids``)."""
    m, n = _prep(masks, n_instances, img_hw)
    B, I, H, W = m.shape
    h, w = _grid_hw(H, W, output_stride)
    if float(sigma) <= 0:
        raise ValueError(f"sigma must be positive, got {sigma}")
    if not _on_device(m):
        cent = _centers_arg(centers, m) if centers is not None else _stats_torch(m, n)[0]
        return _center_torch(m, n, int(output_stride), sigma, cent)
    cent = _centers_arg(centers, m) if centers is not None else torch.empty((B, I, 2), dtype=torch.float32, device=m.device)
    area = torch.empty((B, I), dtype=torch.int64, device=m.device)
    out = torch.empty((B, 1, h, w), dtype=torch.float32, device=m.device)
    _render_device(m, n, output_stride, sigma, False, cent, area, centers is None, center=out)
    return out


def generate_center_offsets(masks: torch.Tensor, img_hw: Optional[Tuple[int, int]] = None, output_stride: int = 2, centers=None, n_instances=None,
                            out: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """-> (offsets (B, 2, h, w) = (cx - x, cy - y) of the instance that owns the cell, weight (B, 1, h, w) = 1 on owned cells); zeros elsewhere.  Both are
    views of one (B, 3, h, w) tensor (``out`` when given): the layout ``SegmentationTrainingModule`` hands to the masked smooth-L1 loss."""
    m, n = _prep(masks, n_instances, img_hw)
    B, I, H, W = m.shape
    h, w = _grid_hw(H, W, output_stride)
    if out is not None:
        _check_out3(out, B, h, w, m.device)
    if not _on_device(m):
        cent, area = _stats_torch(m, n)
        if centers is not None:
            cent = _centers_arg(centers, m)
        return _offsets_torch(m, n, int(output_stride), cent, area, out)
    cent, area = _stats(m, n)
    if centers is not None:
        cent = _centers_arg(centers, m)
    out3 = out if out is not None else torch.empty((B, 3, h, w), dtype=torch.float32, device=m.device)
    _render_device(m, n, output_stride, 1.0, False, cent, area, False, out3=out3)
    return out3[:, :2], out3[:, 2:3]


class SegmentationTargetGenerator:
    """The training targets of ``bottomup_segmentation`` / ``semantic_segmentation``, keyed by head class name plus ``foreground_weight``.

    ``head_config``: the model type's head config; the strides of its heads, ``center.sigma`` and ``segmentation.target_maxpool`` are read from it.
    ``__call__(masks, n_instances)``: ``masks`` (B, I, H, W) uint8 / bool on either device -> ``SegmentationHead`` (B, 1, h, w) and, for
    ``bottomup_segmentation``, ``InstanceCenterHead`` (B, 1, h, w), ``CenterOffsetHead`` (B, 2, h, w) and ``foreground_weight`` (B, 1, h, w); the
    last two are views of one (B, 3, h, w) tensor, which the training module passes on without a copy."""

    def __init__(self, model_type: str, head_config) -> None:
        from sleap_nn_amd.architectures.heads import get_head
        from sleap_nn_amd.utils import cfg_get, to_plain

        if model_type not in SEGMENTATION_TARGET_TYPES:
            raise NotImplementedError(f"'{model_type}' is not a segmentation model type whose targets are rendered here ({', '.join(SEGMENTATION_TARGET_TYPES)}); "
                                      "pose model types take sleap_nn_amd.data.targets.TargetGenerator")
        self.model_type = model_type
        self.heads = {h.name: h for h in get_head(model_type, head_config)}
        seg = to_plain(cfg_get(head_config, "segmentation")) or {}
        self.target_maxpool = bool(seg.get("target_maxpool", False))

    @classmethod
    def from_training_config(cls, cfg_or_path) -> "SegmentationTargetGenerator":
        """From a sleap-nn training config (dict, YAML path or run directory): the non-empty entry of ``model_config.head_configs``."""
        cfg = cfg_or_path
        if isinstance(cfg, (str, os.PathLike)):
            import yaml

            path = os.path.join(cfg, "training_config.yaml") if os.path.isdir(cfg) else cfg
            with open(path) as f:
                cfg = yaml.safe_load(f)
        heads = cfg["model_config"]["head_configs"]
        model_type = next((k for k, v in heads.items() if v), None)
        if model_type is None:
            raise ValueError(f"no head config in the training config: {list(heads)}")
        return cls(model_type, heads[model_type])

    def __call__(self, masks: torch.Tensor, n_instances=None) -> Dict[str, torch.Tensor]:
        H = self.heads
        m, n = _prep(masks, n_instances)
        out = {"SegmentationHead": generate_foreground_mask(m, None, H["SegmentationHead"].output_stride, self.target_maxpool, n)}
        if self.model_type == "bottomup_segmentation":
            cent, _ = _stats(m, n)
            ch, oh = H["InstanceCenterHead"], H["CenterOffsetHead"]
            out["InstanceCenterHead"] = generate_center_heatmap(m, None, ch.output_stride, ch.sigma, cent, n)
            out["CenterOffsetHead"], out["foreground_weight"] = generate_center_offsets(m, None, oh.output_stride, cent, n)
        return out
