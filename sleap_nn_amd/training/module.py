"""One data-parallel training step on the MI355X: forward, per-head MSE (+OHKM), backward,
gradient all-reduce (RCCL over xGMI through ``torch.distributed``), Adam.

Mirrors the step semantics of the reference's LightningModules
(``sleap_nn/training/lightning_modules.py``: ``training_step`` :1850-1922 for bottom-up,
``_compute_negative_weighted_loss`` :490-545 = ``nn.MSELoss`` per head, loss = sum of
``loss_weight`` x head loss, ``compute_ohkm_loss`` ``training/losses.py:8-63``,
``configure_optimizers`` :750-763 = ``torch.optim.Adam(lr, amsgrad)``) and DDP's gradient averaging.
Parameters, gradients and Adam moments live in flat fp32 arenas in the reference's state_dict
order, so the all-reduce is ONE collective over one contiguous buffer (31 MB at cfg3).
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence

import torch
import torch.distributed as dist

from sleap_nn_amd import _lib as L
from sleap_nn_amd.architectures.model import Model


@dataclass
class OHKMConfig:
    """trainer_config.online_hard_keypoint_mining (losses.py:8-15 defaults)."""

    online_mining: bool = False
    hard_to_easy_ratio: float = 2.0
    min_hard_keypoints: int = 2
    max_hard_keypoints: Optional[int] = None
    loss_scale: float = 5.0


class TrainingModule:
    """Owns the device arenas of one model replica and runs training steps."""

    # the segmentation model types train through a subclass that sets their head losses (training/segmentation.py); this class refuses them
    _trains_segmentation = False

    def __init__(self, model: Model, device: str = "cuda", lr: float = 1e-4, betas=(0.9, 0.999), eps: float = 1e-8, amsgrad: bool = False,
                 optimizer: str = "Adam", weight_decay: Optional[float] = None,
                 loss_weights: Optional[Sequence[float]] = None, ohkm: Optional[OHKMConfig] = None,
                 negative_loss_weight: float = 1.0, lr_scheduler=None, max_epochs: Optional[int] = None, wino4: bool = True,
                 native_allreduce: Optional[bool] = None, swint_training: bool = False, stochastic_depth_prob: float = 0.1,
                 stochastic_depth_seed: int = 0, pretrained_training: bool = False, freeze_encoder: Optional[bool] = None) -> None:
        """``negative_loss_weight``: weight of frames flagged ``is_negative`` in the train-stage MSE (lightning_modules.py:149-153,
        526-545).  ``lr_scheduler``: the reference's scheduler config (a name or ``{name: {...}}``, lightning_modules.py:765-857);
        ``self.lr`` then follows it: one ``on_epoch_end(val_loss)`` per epoch, like Lightning steps the scheduler.
        ``wino4``: the K-heavy 3x3 convolutions of the forward and of the data gradients run the Winograd F(4x4,3x3) kernel in the
        training plan too (handle option ``conv_wino4 = 2``; gradients within ~1e-5 of their tensor's scale of the F(2x2,3x3) ones).
        ``native_allreduce``: with more than one rank, exchange the gradients through the C ABI's own RCCL communicator (``ph_model_set_comm``: the two buckets are
        enqueued by ``ph_model_backward`` itself) instead of ``torch.distributed``; default: when the process group's backend is nccl (= RCCL on ROCm).
        ``swint_training``: train a Swin Transformer backbone (opt-in, as ``Model.train(True, allow_swint=True)``).  In the ``"train"`` stage every step then
        draws the per-sample scales of the residual branches on the device -- torchvision's stochastic depth, which the reference trains this backbone with
        (``stochastic_depth_prob`` 0.1, block k dropped with probability ``prob * k / (blocks - 1)``; ``architectures.swint.draw_branch_scales``) -- from a
        generator seeded by ``stochastic_depth_seed``, the rank and the step count; no other stage passes scales, ``stochastic_depth_prob=0`` never does, and
        ``set_branch_scales`` overrides the draw of the next step.
        ``pretrained_training``: train a ``pretrained`` (ConvNeXtV2) backbone (opt-in, as ``Model.train(True, allow_pretrained=True)``): GRN backward and the
        weight gradient of the padding-0 stem on the device; a non-zero ``drop_path_rate`` of the backbone's ``config.json`` is refused.
        ``freeze_encoder``: the reference's ``freeze_encoder()`` for that backbone (lightning_modules.py:232-236); ``None`` takes the backbone config's ``freeze``.
        Frozen, the backward sweep stops behind the decoder (handle option ``bwd_frozen_ops``), every ``backbone.enc.*`` gradient stays exactly zero and the
        optimizer steps only ``Model.trainable_ranges`` of the arena, so neither Adam nor AdamW's decoupled decay moves a frozen parameter.  The same ranges leave
        out the parameters no op reads (``hidden_states_norms.stem``), frozen or not."""
        from sleap_nn_amd.architectures.heads import SEGMENTATION_MODEL_TYPES

        if getattr(model, "model_type", None) in SEGMENTATION_MODEL_TYPES and not self._trains_segmentation:
            raise NotImplementedError(f"training a '{model.model_type}' model is not built here (BCE + Dice, masked smooth-L1 and mask targets): these model types are "
                                      "not trained with the MSE loss of the pose heads; use sleap_nn_amd.training.segmentation.SegmentationTrainingModule")
        self._pretrained = getattr(model, "backbone_type", None) == "pretrained"
        if getattr(model, "is_resnet", False):
            raise NotImplementedError("a 'pretrained' ResNet backbone is inference only on the MI355X path (BatchNorm runs folded into the convs; batch statistics are not built)")
        if getattr(model, "is_swinv2", False):
            raise NotImplementedError("a 'pretrained' Swinv2 backbone is inference only on the MI355X path (its cosine window attention and residual-after-norm LayerNorm have no backward step)")
        if self._pretrained and not pretrained_training:
            raise NotImplementedError("training a 'pretrained' (ConvNeXtV2) backbone is opt-in: TrainingModule(model, pretrained_training=True)")
        if freeze_encoder is not None and not self._pretrained:
            raise ValueError("freeze_encoder freezes the encoder of a 'pretrained' backbone; this model has none")
        if self._pretrained:
            model.backbone.check_trainable()  # (before anything touches the device)
        L.lib()
        if not torch.cuda.is_available():
            raise RuntimeError("TrainingModule needs an MI355X; there is no CPU fallback")
        dev = torch.device(device)
        if dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        self.device = dev
        self._swint = getattr(model, "backbone_type", None) == "swint"
        if self._swint and not swint_training:
            raise NotImplementedError("training a 'swint' backbone is opt-in: TrainingModule(model, swint_training=True)")
        self.stochastic_depth_prob = float(stochastic_depth_prob)
        self.stochastic_depth_seed = int(stochastic_depth_seed)
        if not (0.0 <= self.stochastic_depth_prob < 1.0):
            raise ValueError(f"stochastic_depth_prob must be in [0, 1), got {stochastic_depth_prob}")
        self._next_scales: Optional[torch.Tensor] = None   # set_branch_scales: the next train-stage step's scales instead of a draw
        self._active_scales: Optional[torch.Tensor] = None  # what the handle borrows between the forward and the backward of a step
        self.last_branch_scales: Optional[torch.Tensor] = None  # scales of the last step that had any (kept alive while its kernels run)
        self.model = (model.train(True, allow_swint=True) if self._swint else model.train(True, allow_pretrained=self._pretrained)).to(dev)
        # what the optimizer steps: the whole arena, or -- a pretrained backbone -- what is read and not frozen; the frozen prefix of the backward sweep
        self.frozen_encoder = self._pretrained and bool(model.backbone.freeze if freeze_encoder is None else freeze_encoder)
        self._ranges = model.trainable_ranges(self.frozen_encoder) if self._pretrained else [(0, model.num_parameters())]
        if self._pretrained:
            self.model.set_option("bwd_frozen_ops", model.backbone.encoder_ops() if self.frozen_encoder else 0)
        self.model.set_option("conv_wino4", 2 if wino4 else 1)
        self.lr, self.betas, self.eps, self.amsgrad = lr, betas, eps, amsgrad
        if optimizer not in ("Adam", "AdamW"):
            raise ValueError(f"optimizer must be 'Adam' or 'AdamW' (lightning_modules.py:752-755), got {optimizer!r}")
        # torch's defaults, which is what the reference gets: Adam 0 (L2 form, unused here), AdamW 0.01 (decoupled)
        self.optimizer = optimizer
        self.weight_decay = (0.01 if optimizer == "AdamW" else 0.0) if weight_decay is None else float(weight_decay)
        if optimizer == "Adam" and self.weight_decay != 0.0:
            raise ValueError("Adam with L2 weight decay is not what the reference configures; use optimizer='AdamW'")
        self.loss_weights = [float(w) for w in (loss_weights if loss_weights is not None else [h.loss_weight for h in model.heads])]
        self.ohkm = ohkm or OHKMConfig()
        self.negative_loss_weight = float(negative_loss_weight)
        if isinstance(lr_scheduler, str):  # defaults of the named scheduler (lightning_modules.py:773-785)
            lr_scheduler = {lr_scheduler: {}}
        from sleap_nn_amd.training.schedulers import LRSchedule

        self.schedule = LRSchedule(lr, lr_scheduler, max_epochs) if lr_scheduler else None
        if self.schedule is not None:
            self.lr = self.schedule.lr
        self.params = model.flat_params().to(dev)
        self.grads = torch.zeros_like(self.params)
        self.exp_avg = torch.zeros_like(self.params)
        self.exp_avg_sq = torch.zeros_like(self.params)
        self.max_exp_avg_sq = torch.zeros_like(self.params) if amsgrad else None
        self.step_count = 0
        self._grad_ws: Optional[torch.Tensor] = None
        self._loss = torch.zeros(1 + len(model.heads), dtype=torch.float32, device=dev)
        # from here on the device arena owns the parameters: every (re)compile of the model's handle -- eval() for a
        # validation pass, train() afterwards, a fusion switch -- re-gathers its packed weights from self.params
        self.model.bind_live_params(self.params)
        self.model._ensure(dev)
        self._bucket_split: Optional[int] = None
        self._bucket_event = None
        self._comm_stream = None
        self._comm = None  # the C ABI's RCCL communicator (parallel.Communicator): ph_model_backward then exchanges the gradients itself
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            self._comm_stream = torch.cuda.Stream(dev)
            from sleap_nn_amd.parallel import Communicator

            native = native_allreduce if native_allreduce is not None else (dist.get_backend() == "nccl")
            if native and Communicator.available():
                self._comm = Communicator.create(dev)
            else:  # gloo rehearsals / hosts without librccl: torch.distributed carries the two buckets (parallel.all_reduce_buckets_)
                self._bucket_event = torch.cuda.Event()
                self._bucket_event.record()  # creates the underlying hipEvent_t
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            dist.broadcast(self.params, src=0)  # identical initial weights on every rank (DDP semantics)
            self._push_params()

    # ------------------------------------------------------------------------------
    def _push_params(self) -> None:
        with torch.cuda.device(self.device):
            L.check(L.lib().ph_model_set_params(self.model._handle, C.c_void_p(self.params.data_ptr()), L.current_stream_ptr()))

    def forward_backward(self, image: torch.Tensor, targets: Dict[str, torch.Tensor], is_negative: Optional[torch.Tensor] = None,
                         stage: str = "train") -> torch.Tensor:
        """Forward + loss + backward.  ``image``: (B[,1],C,H,W) uint8/float; ``targets``: head name ->
        (B, c, h, w) fp32.  Fills ``self.grads`` (local gradients) and returns the loss tensor
        ``[total, head_0, head_1, ...]`` (device, no sync).  ``is_negative`` (B,) bool: frames without instances; in the
        train stage their MSE is weighted by ``negative_loss_weight`` (``_compute_negative_weighted_loss``), any other
        stage stays unweighted so ``val/loss`` equals plain ``nn.MSELoss``."""
        x = image.to(self.device, non_blocking=True)
        if x.dim() == 5:
            x = x.squeeze(1)
        code = 0
        if x.dtype != torch.uint8:
            x = x.to(torch.float32)
            code = 2 if bool(x.max() > 1.0) else 1
        if self._pretrained:  # a gray frame is replicated here, as Model.forward would: the backward reads the frames the stem saw
            x, code = self.model.adapt_channels(x, code)
        x = x.contiguous()
        B, Cin, H, W = x.shape
        lib = L.lib()
        m = self.model
        self._bind_branch_scales(B, stage)
        try:
            return self._forward_backward(x, code, targets, is_negative, stage)
        finally:  # borrowed until the backward has been enqueued: a later eval() / validation forward sees none
            if self._active_scales is not None and getattr(m, "_handle", None) is not None:
                lib.ph_model_set_branch_scales(m._handle, None, 0, 0)
            self._active_scales = None

    def set_branch_scales(self, scales: Optional[torch.Tensor]) -> None:
        """Scales of the residual branches for the NEXT train-stage step instead of a draw: ``(n_branches, B)``, rows in program order (attention branch, then MLP
        branch, of each block); ``None`` withdraws an override that has not been used yet."""
        self._next_scales = None if scales is None else torch.as_tensor(scales, dtype=torch.float32).to(self.device).contiguous()

    def _bind_branch_scales(self, B: int, stage: str) -> None:
        if not self._swint or stage != "train":
            return
        scales, self._next_scales = self._next_scales, None
        if scales is None and self.stochastic_depth_prob > 0.0:
            from sleap_nn_amd.architectures.swint import draw_branch_scales

            rank = dist.get_rank() if dist.is_available() and dist.is_initialized() else 0
            g = torch.Generator(device=self.device)
            g.manual_seed((self.stochastic_depth_seed * 1000003 + rank) * 1000003 + self.step_count)
            scales = draw_branch_scales(self.model.backbone.depths, B, self.stochastic_depth_prob, generator=g, device=self.device)
        if scales is None:
            return
        m = self.model
        n = m.residual_branches()
        if tuple(scales.shape) != (n, B):
            raise ValueError(f"branch scales have shape {tuple(scales.shape)}, the step needs ({n}, {B})")
        m._ensure(self.device)
        with torch.cuda.device(self.device):
            L.check(L.lib().ph_model_set_branch_scales(m._handle, C.c_void_p(scales.data_ptr()), n, B))
        self._active_scales = self.last_branch_scales = scales

    def _forward_backward(self, x: torch.Tensor, code: int, targets: Dict[str, torch.Tensor], is_negative, stage: str) -> torch.Tensor:
        out = self.model.forward(x, in_dtype=None if code == 0 else code)
        B, Cin, H, W = x.shape
        lib = L.lib()
        m = self.model
        with torch.cuda.device(self.device):
            need = L.check(lib.ph_model_backward_workspace_bytes(m._handle, B, H, W))
            if self._grad_ws is None or self._grad_ws.numel() < need:
                self._grad_ws = None
                self._grad_ws = torch.empty(int(need), dtype=torch.uint8, device=self.device)
            outs = [out[h.name].contiguous() for h in m.heads]
            tg = [targets[h.name].to(self.device, torch.float32).contiguous() for h in m.heads]
            for i, (o, t) in enumerate(zip(outs, tg)):
                if tuple(t.shape) != self._target_shape(i, tuple(o.shape)):
                    raise ValueError(f"target shape {tuple(t.shape)} != {self._target_shape(i, tuple(o.shape))} for a prediction of shape {tuple(o.shape)}")
            optr = (C.c_void_p * len(outs))(*[o.data_ptr() for o in outs])
            tptr = (C.c_void_p * len(tg))(*[t.data_ptr() for t in tg])
            lw = (C.c_float * len(self.loss_weights))(*self.loss_weights)
            sw = None
            if is_negative is not None and stage == "train" and self.negative_loss_weight != 1.0:
                neg = torch.as_tensor(is_negative).to(self.device).reshape(-1).bool()
                if neg.numel() != B:
                    raise ValueError(f"is_negative has {neg.numel()} entries for a batch of {B}")
                sw = torch.where(neg, float(self.negative_loss_weight), 1.0).to(torch.float32).contiguous()
            k = self.ohkm
            # (re)bind on every step: the handle may have been recompiled, or last used by another TrainingModule whose event
            # is gone -- a handle never keeps an event this module does not own (NULL = no mid-sweep record)
            if self._bucket_event is not None:
                self._bucket_split = int(L.check(lib.ph_model_grad_bucket_split(m._handle)))
                L.check(lib.ph_model_set_bucket_event(m._handle, C.c_void_p(self._bucket_event.cuda_event)))
            else:
                L.check(lib.ph_model_set_bucket_event(m._handle, None))
            # (the native exchange: bound per step for the same reason; validation passes compute no exchange -- every rank evaluates its own shard)
            if self._comm is not None and stage == "train":
                L.check(lib.ph_model_set_comm(m._handle, C.c_void_p(self._comm.handle), C.c_void_p(self._comm_stream.cuda_stream)))
            else:
                L.check(lib.ph_model_set_comm(m._handle, None, None))
            L.check(
                lib.ph_model_backward(
                    m._handle, C.c_void_p(x.data_ptr()), code, B, Cin, H, W, C.c_void_p(m._workspace.data_ptr()), C.c_void_p(self._grad_ws.data_ptr()),
                    self._grad_ws.numel(), optr, tptr, lw, C.c_void_p(sw.data_ptr()) if sw is not None else None, 1 if k.online_mining else 0, float(k.hard_to_easy_ratio), int(k.min_hard_keypoints),
                    -1 if k.max_hard_keypoints is None else int(k.max_hard_keypoints), float(k.loss_scale), C.c_void_p(self._loss.data_ptr()),
                    C.c_void_p(self.grads.data_ptr()), L.current_stream_ptr(),
                )
            )
        self._last_out = out
        return self._loss

    def padded_token_vector(self, batch: int, height: int, width: int) -> torch.Tensor:
        """Swin programs: the (3C) share of ``qkv.bias``'s gradient that came through the padded tokens of the program's first attention op in the last
        ``forward_backward`` of this shape (``ph_model_backward_pad_vector``): exactly zero where the map needs no padding."""
        n = C.c_int32()
        off = L.check(L.lib().ph_model_backward_pad_vector(self.model._handle, batch, height, width, C.byref(n)))
        return self._grad_ws[int(off) : int(off) + 4 * n.value].view(torch.float32).clone()

    def _target_shape(self, head_index: int, pred_shape: tuple) -> tuple:
        """Shape of head ``head_index``'s target for a prediction of ``pred_shape`` (a subclass's loss may take more channels)."""
        return pred_shape

    def all_reduce_grads(self) -> float:
        """Sum the flat gradient arena over the ranks; returns the scale that turns the sum into DDP's mean.

        Two buckets, overlapped with the backward sweep: the arena tail (decoder + heads, final first) is reduced on a side
        stream as soon as the backward has recorded ``_bucket_event`` -- while the encoder's gradients are still being
        computed -- and the head of the arena right after the backward; the compute stream waits for both before Adam.  On
        xGMI a ring all-reduce is bound by one link (~153 GB/s): 31 MB (cfg3 UNet) / 352 MB (ConvNeXt-tiny) take ~0.4 / ~4 ms,
        so one bucket boundary is all the overlap there is to win."""
        if self._comm is not None:  # ph_model_backward has already enqueued both buckets (ph_model_set_comm) and joined the side stream
            return 1.0 / self._comm.world
        from sleap_nn_amd.parallel import all_reduce_buckets_

        return all_reduce_buckets_(self.grads, self._bucket_split, tail_ready=self._bucket_event, comm_stream=self._comm_stream)

    def optimizer_step(self, grad_scale: float = 1.0) -> None:
        self.step_count += 1
        with torch.cuda.device(self.device):
            for lo, hi in self._ranges:  # (one range, the whole arena, unless a pretrained backbone leaves parameters out)
                p = lambda t: C.c_void_p(t.data_ptr() + 4 * lo)  # noqa: E731
                L.check(
                    L.lib().ph_adamw_step(
                        p(self.params), p(self.grads), p(self.exp_avg), p(self.exp_avg_sq), p(self.max_exp_avg_sq) if self.max_exp_avg_sq is not None else None,
                        hi - lo, float(self.lr), float(self.betas[0]), float(self.betas[1]), float(self.eps), float(self.weight_decay), self.step_count,
                        float(grad_scale), L.current_stream_ptr(),
                    )
                )
        self._push_params()

    def training_step(self, batch: Dict[str, torch.Tensor]) -> torch.Tensor:
        """``batch``: {"image": ..., <head name>: target, ..., ["is_negative": (B,) bool]}.  Returns the loss tensor (device)."""
        targets = {k: v for k, v in batch.items() if k not in ("image", "is_negative")}
        loss = self.forward_backward(batch["image"], targets, batch.get("is_negative"))
        scale = self.all_reduce_grads()
        self.optimizer_step(scale)
        return loss

    def validation_step(self, batch: Dict[str, torch.Tensor]) -> torch.Tensor:
        """Loss of a validation batch on the current parameters: unweighted (``stage="val"``), no optimizer step.  The
        gradients it leaves in ``self.grads`` are overwritten by the next training step."""
        targets = {k: v for k, v in batch.items() if k not in ("image", "is_negative")}
        return self.forward_backward(batch["image"], targets, batch.get("is_negative"), stage="val").clone()

    def on_epoch_end(self, val_loss: Optional[float] = None) -> float:
        """Step the learning-rate schedule once (Lightning: interval "epoch", monitor "val/loss"); returns the next epoch's lr."""
        if self.schedule is not None:
            self.lr = self.schedule.step(val_loss)
        return self.lr

    def close(self) -> None:
        """Unbind this module's bucket event from the model handle (the handle may outlive the module)."""
        ev, self._bucket_event = self._bucket_event, None
        if ev is not None and getattr(self.model, "_handle", None) is not None:
            L.lib().ph_model_set_bucket_event(self.model._handle, None)
        comm, self._comm = getattr(self, "_comm", None), None
        if comm is not None:
            if getattr(self.model, "_handle", None) is not None:
                L.lib().ph_model_set_comm(self.model._handle, None, None)
            comm.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------------------------
    def named_grads(self) -> Dict[str, torch.Tensor]:
        out, o = {}, 0
        g = self.grads.detach().cpu()
        for k in self.model.param_keys():
            n = int(torch.tensor(self.model.param_shapes[k]).prod())
            out[k] = g[o : o + n].reshape(self.model.param_shapes[k])
            o += n
        return out

    def state_dict(self) -> Dict[str, torch.Tensor]:
        self.model.load_flat_params(self.params)
        return self.model.state_dict()
