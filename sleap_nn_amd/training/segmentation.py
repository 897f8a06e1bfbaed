"""Training step of the segmentation model types on the MI355X.

Mirrors ``BottomUpSegmentationLightningModule.training_step`` and ``SemanticSegmentationLightningModule.training_step``
(``sleap_nn/training/lightning_modules.py:3052-3109, 3463-3475``): BCE + Dice on the foreground LOGITS (``compute_bce_dice_loss``),
``F.mse_loss`` on the centre map, masked smooth-L1 on the centre offsets, total = sum of ``loss_weight`` x head loss.  The backbone
backward, Adam, the schedules and the gradient exchange are ``TrainingModule``'s; this class only chooses each head's loss on the
model's handle (``Model.set_head_loss`` -> ``ph_model_set_head_loss``) and packs the offsets and their weight mask into the
``(B, 3, h, w)`` target the smooth-L1 kernel takes.

In training the model's ``SegmentationHead`` output is the logit map (the reference supervises ``self.model(X)``, not its ``forward``);
after ``model.eval()`` a forward returns probabilities again.
"""
from __future__ import annotations

from typing import Dict, Optional

import torch

from sleap_nn_amd import _lib as L
from sleap_nn_amd.architectures.heads import SEGMENTATION_MODEL_TYPES
from sleap_nn_amd.architectures.model import Model
from sleap_nn_amd.training.module import OHKMConfig, TrainingModule
from sleap_nn_amd.utils import cfg_get, to_plain

DICE_SMOOTH = 1.0  # compute_bce_dice_loss's default, which the reference's training steps never override


class SegmentationTrainingModule(TrainingModule):
    """``TrainingModule`` for ``bottomup_segmentation`` and ``semantic_segmentation`` models.

    ``bce_weight`` / ``dice_weight`` (default 0.5 each) and ``bce_pos_weight`` (default None) come from the ``segmentation`` leaf of the model's head
    config, ``loss_weight`` from each head.  A batch is ``{"image", "SegmentationHead"[, "InstanceCenterHead", "CenterOffsetHead",
    "foreground_weight"]}``: what ``SegmentationTargetGenerator`` returns beside the image.  Every other keyword is ``TrainingModule``'s and is passed through:
    ``pretrained_training=True`` (with ``freeze_encoder``) trains a model on a ``pretrained`` (ConvNeXtV2) backbone, ``swint_training=True`` one on a Swin backbone."""

    _trains_segmentation = True

    def __init__(self, model: Model, device: str = "cuda", ohkm: Optional[OHKMConfig] = None, negative_loss_weight: float = 1.0, **kwargs) -> None:
        mt = getattr(model, "model_type", None)
        if mt not in SEGMENTATION_MODEL_TYPES:
            raise ValueError(f"SegmentationTrainingModule trains {', '.join(SEGMENTATION_MODEL_TYPES)} models, not '{mt}': use TrainingModule")
        if ohkm is not None and ohkm.online_mining:
            raise ValueError("online hard keypoint mining ranks keypoint channels: the segmentation losses have none (the reference's segmentation steps ignore it)")
        if float(negative_loss_weight) != 1.0:
            raise ValueError("negative_loss_weight weighs the MSE of pose heads; the segmentation losses are not weighted per frame")
        seg = to_plain(cfg_get(model.head_configs, "segmentation")) or {}
        self.bce_weight = float(seg.get("bce_weight", 0.5))
        self.dice_weight = float(seg.get("dice_weight", 0.5))
        pw = seg.get("bce_pos_weight", None)
        self.bce_pos_weight = None if pw is None else float(pw)
        if self.bce_pos_weight is not None and self.bce_pos_weight < 0:
            raise ValueError(f"bce_pos_weight must not be negative, got {pw}")
        self._offset_index = None
        for i, h in enumerate(model.heads):
            if h.loss_function == "bce_dice":
                model.set_head_loss(i, L.LOSS_BCE_DICE, (self.bce_weight, self.dice_weight, DICE_SMOOTH, -1.0 if self.bce_pos_weight is None else self.bce_pos_weight))
            elif h.loss_function == "smooth_l1":
                model.set_head_loss(i, L.LOSS_MASKED_SMOOTH_L1)
                self._offset_index = i
            else:
                model.set_head_loss(i, L.LOSS_MSE)
        super().__init__(model, device, ohkm=None, negative_loss_weight=1.0, **kwargs)

    def _target_shape(self, head_index: int, pred_shape: tuple) -> tuple:
        if head_index == self._offset_index:  # the offsets, then their weight mask
            return (pred_shape[0], pred_shape[1] + 1) + tuple(pred_shape[2:])
        return pred_shape

    def forward_backward(self, image: torch.Tensor, targets: Dict[str, torch.Tensor], is_negative: Optional[torch.Tensor] = None, stage: str = "train") -> torch.Tensor:
        """As ``TrainingModule.forward_backward``; ``targets`` also holds ``foreground_weight`` (B, 1, h, w) when the model has a ``CenterOffsetHead``."""
        targets = dict(targets)
        if self._offset_index is not None:
            name = self.model.heads[self._offset_index].name
            off, wt = targets[name], targets.pop("foreground_weight", None)
            if wt is None:
                if off.shape[1] != 3:
                    raise ValueError(f"targets need 'foreground_weight' beside '{name}' (or '{name}' packed as (B, 3, h, w))")
            else:
                base = off._base
                packed = (base is not None and base is wt._base and base.dim() == 4 and base.shape[1] == 3 and base.is_contiguous() and base.dtype == torch.float32
                          and off.data_ptr() == base.data_ptr() and off.shape[1] == 2 and wt.data_ptr() == base.data_ptr() + 8 * base.shape[2] * base.shape[3]
                          and off.stride() == base.stride() and wt.stride() == base.stride())
                # (the generator rendered both into one buffer: no copy)
                targets[name] = base if packed else torch.cat([off.to(torch.float32), wt.to(off.device, torch.float32)], dim=1)
        return super().forward_backward(image, targets, None, stage)
