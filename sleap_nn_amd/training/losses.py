"""Losses of the segmentation model types, with the reference's names, arguments and defaults
(``sleap_nn/training/losses.py:64-133``: ``compute_bce_dice_loss``, ``compute_masked_smooth_l1``).

They dispatch on the device, as ``data/targets.py`` does: tensors on the GPU take the HIP kernels (``ph_loss_bce_dice``,
``ph_loss_masked_smooth_l1``: fixed-order partial sums, bitwise reproducible), CPU tensors a torch form of the same contract,
which is what the CPU tests pin against the reference's recorded values.  The ``*_with_grad`` variants also return the gradient
with respect to the prediction; ``ph_model_backward`` runs the same kernels for heads whose loss was chosen with
``Model.set_head_loss``.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Tuple

import torch
import torch.nn.functional as F

from sleap_nn_amd import _lib as L


def _bce_dice_torch(y_pred, y_gt, bce_weight, dice_weight, smooth, pos_weight):
    pw = None if pos_weight is None else torch.as_tensor(pos_weight, dtype=y_pred.dtype, device=y_pred.device)
    bce = F.binary_cross_entropy_with_logits(y_pred, y_gt, reduction="mean", pos_weight=pw)
    p = torch.sigmoid(y_pred)
    inter = (p * y_gt).sum(dim=(2, 3))
    union = p.sum(dim=(2, 3)) + y_gt.sum(dim=(2, 3))
    dice = (2.0 * inter + smooth) / (union + smooth)
    return bce_weight * bce + dice_weight * (1.0 - dice.mean())


def _masked_smooth_l1_torch(y_pred, y_gt, mask):
    m = mask.expand_as(y_pred)
    n_valid = m.sum()
    if n_valid == 0:
        return (y_pred * 0.0).sum()  # exactly 0, and a zero gradient
    return F.smooth_l1_loss(y_pred * m, y_gt * m, reduction="sum") / n_valid


def _scratch(B: int, Cn: int, device) -> torch.Tensor:
    n = L.check(L.lib().ph_loss_scratch_bytes(int(B), int(Cn)))
    return torch.empty(int(n), dtype=torch.uint8, device=device)


def _check_maps(name, y_pred, y_gt):
    if y_pred.dim() != 4 or tuple(y_gt.shape) != tuple(y_pred.shape):
        raise ValueError(f"{name}: prediction {tuple(y_pred.shape)} and target {tuple(y_gt.shape)} must be the same (B, C, H, W)")


def compute_bce_dice_loss_with_grad(y_pred: torch.Tensor, y_gt: torch.Tensor, bce_weight: float = 0.5, dice_weight: float = 0.5, smooth: float = 1.0,
                                    pos_weight: Optional[float] = None, loss_weight: float = 1.0) -> Tuple[torch.Tensor, torch.Tensor]:
    """-> (loss, ``loss_weight`` x d loss / d ``y_pred``).  ``y_pred``: logits (B, 1, H, W); ``y_gt``: binary mask of the same shape."""
    _check_maps("compute_bce_dice_loss", y_pred, y_gt)
    if y_pred.shape[1] != 1:
        raise ValueError(f"compute_bce_dice_loss: one channel of logits expected, got {tuple(y_pred.shape)}")
    if not y_pred.is_cuda or y_pred.numel() == 0:
        z = y_pred.detach().to(torch.float32).requires_grad_(True)
        loss = _bce_dice_torch(z, y_gt.to(torch.float32), bce_weight, dice_weight, smooth, pos_weight)
        (g,) = torch.autograd.grad(loss, z)
        return loss.detach(), g * loss_weight
    z = y_pred.detach().to(torch.float32).contiguous()
    t = y_gt.detach().to(z.device, torch.float32).contiguous()
    B, _, H, W = z.shape
    loss = torch.empty(1, dtype=torch.float32, device=z.device)
    grad = torch.empty_like(z)
    with torch.cuda.device(z.device):
        ws = _scratch(B, 1, z.device)
        L.check(L.lib().ph_loss_bce_dice(C.c_void_p(z.data_ptr()), C.c_void_p(t.data_ptr()), B, H, W, float(bce_weight), float(dice_weight), float(smooth),
                                         -1.0 if pos_weight is None else float(pos_weight), float(loss_weight), C.c_void_p(loss.data_ptr()),
                                         C.c_void_p(grad.data_ptr()), C.c_void_p(ws.data_ptr()), ws.numel(), L.current_stream_ptr()))
    return loss[0], grad


def compute_bce_dice_loss(y_pred: torch.Tensor, y_gt: torch.Tensor, bce_weight: float = 0.5, dice_weight: float = 0.5, smooth: float = 1.0,
                          pos_weight: Optional[float] = None) -> torch.Tensor:
    """Binary cross entropy (with logits, mean) plus Dice (per sample, ``1 - mean``), weighted.  CPU tensors: the torch form, differentiable."""
    if not y_pred.is_cuda:
        _check_maps("compute_bce_dice_loss", y_pred, y_gt)
        return _bce_dice_torch(y_pred, y_gt, bce_weight, dice_weight, smooth, pos_weight)
    return compute_bce_dice_loss_with_grad(y_pred, y_gt, bce_weight, dice_weight, smooth, pos_weight)[0]


def compute_masked_smooth_l1_with_grad(y_pred: torch.Tensor, y_gt: torch.Tensor, mask: torch.Tensor, loss_weight: float = 1.0) -> Tuple[torch.Tensor, torch.Tensor]:
    """-> (loss, ``loss_weight`` x d loss / d ``y_pred``).  ``mask``: (B, 1, H, W) binary, broadcast over the channels."""
    _check_maps("compute_masked_smooth_l1", y_pred, y_gt)
    if tuple(mask.shape) != (y_pred.shape[0], 1) + tuple(y_pred.shape[2:]):
        raise ValueError(f"compute_masked_smooth_l1: mask {tuple(mask.shape)} must be (B, 1, H, W) of the prediction {tuple(y_pred.shape)}")
    if not y_pred.is_cuda or y_pred.numel() == 0:
        p = y_pred.detach().to(torch.float32).requires_grad_(True)
        loss = _masked_smooth_l1_torch(p, y_gt.to(torch.float32), mask.to(torch.float32))
        (g,) = torch.autograd.grad(loss, p)
        return loss.detach(), g * loss_weight
    p = y_pred.detach().to(torch.float32).contiguous()
    t = y_gt.detach().to(p.device, torch.float32).contiguous()
    m = mask.detach().to(p.device, torch.float32).contiguous()
    B, Cn, H, W = p.shape
    loss = torch.empty(1, dtype=torch.float32, device=p.device)
    grad = torch.empty_like(p)
    with torch.cuda.device(p.device):
        ws = _scratch(B, Cn, p.device)
        L.check(L.lib().ph_loss_masked_smooth_l1(C.c_void_p(p.data_ptr()), C.c_void_p(t.data_ptr()), C.c_void_p(m.data_ptr()), B, Cn, H, W, float(loss_weight),
                                                 C.c_void_p(loss.data_ptr()), C.c_void_p(grad.data_ptr()), C.c_void_p(ws.data_ptr()), ws.numel(), L.current_stream_ptr()))
    return loss[0], grad


def compute_masked_smooth_l1(y_pred: torch.Tensor, y_gt: torch.Tensor, mask: torch.Tensor) -> torch.Tensor:
    """Smooth-L1 (beta 1) of ``mask * y_pred`` against ``mask * y_gt``, summed, over the number of valid elements; 0 when there is none."""
    if not y_pred.is_cuda:
        _check_maps("compute_masked_smooth_l1", y_pred, y_gt)
        return _masked_smooth_l1_torch(y_pred, y_gt, mask)
    return compute_masked_smooth_l1_with_grad(y_pred, y_gt, mask)[0]
