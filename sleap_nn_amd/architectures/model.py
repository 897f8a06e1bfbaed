"""``Model`` = backbone + heads, executed by libposehip on an MI355X.

Drop-in for ``sleap_nn.architectures.model.Model`` (architectures/model.py:157-261): same
constructor signature, same ``state_dict`` key names (so reference checkpoints load), same
``forward(x) -> {head class name: (B, C, H/s, W/s) fp32 NCHW tensor}``.  There are no torch
modules underneath: weights are re-packed once and the forward is one C-ABI call that
enqueues hand-written gfx950 kernels on the current torch stream.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional

import torch

from sleap_nn_amd import _lib as L
from sleap_nn_amd.architectures.heads import SEGMENTATION_MODEL_TYPES, ClassMapsHead, ClassVectorsHead, Head, SegmentationHead, get_head
from sleap_nn_amd.architectures.convnext import ConvNextWrapper
from sleap_nn_amd.architectures.pretrained import PretrainedBackbone
from sleap_nn_amd.architectures.swint import SwinTWrapper
from sleap_nn_amd.architectures.unet import OpSpec, UNet
from sleap_nn_amd.utils import cfg_get, cfg_keys


PRECISIONS = {"exact": 0, "split": 1, "fp16": 2}


def get_backbone(backbone: str, backbone_config):
    """architectures/model.py:36-67.  ``unet``, ``convnext``, ``swint`` and ``pretrained`` (the ConvNeXtV2 family; the ResNet family with the config key
    ``allow_resnet`` and the Swinv2 family with ``allow_swinv2``, both inference only) are built natively; all four train on the device."""
    if backbone == "unet":
        return UNet.from_config(backbone_config)
    if backbone == "convnext":
        return ConvNextWrapper.from_config(backbone_config)
    if backbone == "swint":
        return SwinTWrapper.from_config(backbone_config)
    if backbone == "pretrained":
        return PretrainedBackbone.from_config(backbone_config)
    raise KeyError(f"Unsupported backbone: {backbone}. Supported backbones are: unet, convnext, swint, pretrained")


class Model:
    """Backbone + 1x1 heads (architectures/model.py:157-261)."""

    def __init__(self, backbone_type: str, backbone_config, head_configs, model_type: str) -> None:
        self.backbone_type = backbone_type
        self.backbone_config = backbone_config
        self.head_configs = head_configs
        self.model_type = model_type
        self.heads: List[Head] = get_head(model_type, head_configs)
        self.backbone: UNet = get_backbone(backbone_type, backbone_config)
        self.in_channels = int(cfg_get(backbone_config, "in_channels", 3 if backbone_type == "pretrained" else 1))

        self.ops: List[OpSpec] = list(self.backbone.ops)
        self.param_shapes = dict(self.backbone.param_shapes)
        # checkpoint entries that are not parameters, kept out of the parameter arena: Swin's relative_position_index is checked at load; the
        # `loaded_buffers` of a pretrained backbone (image_mean / image_std) are read from the checkpoint and handed to the handle (ph_model_set_input_norm)
        self.buffers: Dict[str, torch.Tensor] = dict(getattr(self.backbone, "buffers", {}))
        self._loaded_buffers = tuple(getattr(self.backbone, "loaded_buffers", ()))
        self._ignored_buffers = tuple(getattr(self.backbone, "ignored_buffers", ()))  # in every checkpoint, accepted, never read (BatchNorm's num_batches_tracked)
        self._head_ops_start = len(self.ops)
        for i, head in enumerate(self.heads):
            if isinstance(head, ClassVectorsHead):
                self._add_class_vector_head(i, head)
                continue
            s2f = self.backbone.decoder_stride_to_filters
            if head.output_stride not in self.backbone.decoder_slot_of_stride:
                if not self.backbone.decoder_slot_of_stride and head.output_stride in s2f:
                    src = self.backbone.middle_slot
                else:
                    raise ValueError(
                        f"Head '{head.name}' needs a feature map at output_stride {head.output_stride}, "
                        f"backbone produces strides {sorted(self.backbone.decoder_slot_of_stride)}"
                    )
            else:
                src = self.backbone.decoder_slot_of_stride[head.output_stride]
            cin = s2f[head.output_stride]
            name = f"head_layers.{i}.{head.name}.0"
            self.param_shapes[name + ".weight"] = (head.channels, cin, 1, 1)
            self.param_shapes[name + ".bias"] = (head.channels,)
            flags = L.FLAG_SIGMOID if isinstance(head, ClassMapsHead) else 0
            if model_type in SEGMENTATION_MODEL_TYPES:
                # the reference applies the foreground sigmoid in the Lightning module's forward (lightning_modules.py:3041-3050): here it is the head op's epilogue,
                # so the output dict equals that forward's -- probabilities under "SegmentationHead", raw maps under the other keys.  Inference only (PH_FLAG_NO_TRAIN).
                flags = (L.FLAG_SIGMOID if isinstance(head, SegmentationHead) else 0) | L.FLAG_NO_TRAIN
            self.ops.append(OpSpec(L.OP_HEAD, src, -1, -1, cin, 0, head.channels, 1, flags, name + ".weight", name + ".bias", out_index=i, label=name))
        self.unfused_ops = list(self.ops)
        self.fused_ops = self._fuse_cnblocks(self._fuse_pools(self._fuse_stem(self.ops)))
        self.ops = self.fused_ops
        self._state: Dict[str, torch.Tensor] = {k: torch.zeros(v, dtype=torch.float32) for k, v in self.param_shapes.items()}
        self._handle = None
        self._handle_device: Optional[torch.device] = None
        self._workspace: Optional[torch.Tensor] = None
        self.device = torch.device("cpu")
        # bumped whenever the native handle or the workspace is replaced: anything that captured raw pointers into them
        # (HipBackend's hipGraphs) compares generations before replaying
        self.generation = 0
        self._options: Dict[str, float] = {}
        self.precision = "exact"
        self.keep_activations = False
        self._last_batch = 0  # batch of the last forward (read_slot)
        # a TrainingModule registers its device parameter arena here; after any recompile the packed weights are
        # re-gathered from it, so eval()/train() round trips never fall back to the host copy in _state
        self._live_params: Optional[torch.Tensor] = None
        self._options["workspace_reuse"] = 1.0  # the model starts in the inference (fused) program
        # head index -> (PH_LOSS_* kind, parameters): set_head_loss; applied to every training handle, never to an inference one
        self._head_losses: Dict[int, tuple] = {}

    def _add_class_vector_head(self, i: int, head: "ClassVectorsHead") -> None:
        """heads.py:506-539 on the decoder's input feature (architectures/model.py:197-199,253-255)."""
        if not head.global_pool:
            raise ValueError("ClassVectorsHead without global_pool is not supported (the reference flattens a fixed-size feature map)")
        bbn = self.backbone
        src = bbn.middle_slot
        cin = int(bbn.max_channels)
        dst = bbn._new_slot()
        self.ops.append(OpSpec(L.OP_GLOBAL_MAXPOOL, src, -1, dst, cin, label=f"head_layers.{i}.pre_classification_global_pool"))
        cur, cur_c = dst, cin
        for j in range(head.num_fc_layers):
            name = f"head_layers.{i}.pre_classification{j}_fc"
            self.param_shapes[name + ".weight"] = (head.num_fc_units, cur_c)
            self.param_shapes[name + ".bias"] = (head.num_fc_units,)
            dst = bbn._new_slot()
            self.ops.append(OpSpec(L.OP_LINEAR, cur, -1, dst, cur_c, 0, head.num_fc_units, 1, L.FLAG_RELU, name + ".weight", name + ".bias", label=name))
            cur, cur_c = dst, head.num_fc_units
        name = f"head_layers.{i}.{head.name}"
        self.param_shapes[name + ".weight"] = (head.channels, cur_c)
        self.param_shapes[name + ".bias"] = (head.channels,)
        self.ops.append(OpSpec(L.OP_HEAD, cur, -1, -1, cur_c, 0, head.channels, 1, L.FLAG_SOFTMAX, name + ".weight", name + ".bias", out_index=i, label=name))

    @staticmethod
    def _fuse_stem(ops: List[OpSpec]) -> List[OpSpec]:
        """Plan-level fusion of the first encoder block: INPUT_CONV -> CONV -> POOL becomes one
        PH_OP_STEM launch when both convs have <= 16 filters (the full-resolution activations then
        never round-trip through HBM; the full-res output is still written if a decoder block or a
        head reads it)."""
        if len(ops) < 3:
            return ops
        a, b, c = ops[0], ops[1], ops[2]
        ok = (
            a.kind == L.OP_INPUT_CONV and b.kind == L.OP_CONV and c.kind == L.OP_POOL and b.src0 == a.dst and b.src1 < 0
            and c.src0 == b.dst and a.cout <= 16 and b.cout <= 16 and a.cin0 in (1, 3) and a.ksize == 3 and b.ksize == 3
            and not any(o.src0 == a.dst or o.src1 == a.dst for o in ops[2:])
        )
        if not ok:
            return ops
        full_needed = any(o.src0 == b.dst or o.src1 == b.dst for o in ops[3:])
        fused = OpSpec(
            L.OP_STEM, -1, -1, b.dst if full_needed else -1, a.cin0, 0, b.cout, 3, L.FLAG_RELU, a.weight, a.bias,
            label=b.label + "+pool(fused stem)", dst2=c.dst, weight2=b.weight, bias2=b.bias, cmid=a.cout,
        )
        return [fused] + ops[3:]

    @staticmethod
    def _fuse_pools(ops: List[OpSpec]) -> List[OpSpec]:
        """CONV(+ReLU) followed by the POOL of its output -> the conv's epilogue also writes the
        pooled tensor (``dst2``); the full-resolution output is still written (it is the skip)."""
        import copy

        out: List[OpSpec] = []
        i = 0
        while i < len(ops):
            op = ops[i]
            nxt = ops[i + 1] if i + 1 < len(ops) else None
            if op.kind == L.OP_CONV and (op.flags & L.FLAG_RELU) and op.dst2 < 0 and nxt is not None and nxt.kind == L.OP_POOL and nxt.src0 == op.dst:
                f = copy.copy(op)
                f.dst2 = nxt.dst
                f.label = op.label + "+pool"
                out.append(f)
                i += 2
                continue
            out.append(op)
            i += 1
        return out

    @staticmethod
    def _fuse_cnblocks(ops: List[OpSpec]) -> List[OpSpec]:
        """LINEAR -> GELU and LINEAR -> SCALE_ADD pairs become one row GEMM with the activation /
        ``layer_scale * u + x`` in its epilogue (the 4C-wide pre-activation and the un-scaled block
        output then never exist in HBM)."""
        import copy

        def readers(slot, skip):
            return [o for o in ops if o is not skip and (o.src0 == slot or o.src1 == slot)]

        out: List[OpSpec] = []
        i = 0
        while i < len(ops):
            op = ops[i]
            nxt = ops[i + 1] if i + 1 < len(ops) else None
            if op.kind == L.OP_LINEAR and op.flags == 0 and nxt is not None and nxt.src0 == op.dst and not readers(op.dst, nxt):
                if nxt.kind == L.OP_GELU:
                    f = copy.copy(op)
                    f.flags, f.dst = L.FLAG_GELU, nxt.dst
                    out.append(f)
                    i += 2
                    continue
                if nxt.kind == L.OP_SCALE_ADD:
                    f = copy.copy(op)
                    f.flags, f.dst, f.src1, f.weight2, f.label = L.FLAG_SCALE_RESIDUAL, nxt.dst, nxt.src1, nxt.weight, nxt.label
                    out.append(f)
                    i += 2
                    continue
            out.append(op)
            i += 1
        return out

    @classmethod
    def from_config(cls, backbone_type, backbone_config, head_configs, model_type) -> "Model":
        return cls(backbone_type, backbone_config, head_configs, model_type)

    # -- parameters -----------------------------------------------------------------------
    def state_dict(self) -> Dict[str, torch.Tensor]:
        return {**self._state, **self.buffers}

    def load_state_dict(self, state_dict: Dict[str, torch.Tensor], strict: bool = True):
        """Accepts ``Model`` keys or LightningModule keys (``model.`` prefix, loaders.py:144-176)."""
        sd = {}
        for k, v in state_dict.items():
            k = k[len("model.") :] if k.startswith("model.") else k
            sd[k] = v
        missing = [k for k in self.param_shapes if k not in sd]
        missing += [k for k in self.buffers if k not in sd]
        unexpected = [k for k in sd if k not in self.param_shapes and k not in self.buffers]
        if strict and (missing or unexpected):
            raise RuntimeError(f"Error(s) in loading state_dict: missing {missing}, unexpected {unexpected}")
        for k, want in self.buffers.items():
            if k in sd and k in self._loaded_buffers:  # the checkpoint's values are the ones the run was trained with: used, whatever the config would have given
                got = torch.as_tensor(sd[k]).detach().to("cpu", torch.float32).contiguous()
                if tuple(got.shape) != tuple(want.shape):
                    raise RuntimeError(f"size mismatch for {k}: checkpoint {tuple(got.shape)} vs model {tuple(want.shape)}")
                self.buffers[k] = got.clone()
            elif k in sd and k in self._ignored_buffers:
                continue
            elif k in sd:  # the kernels compute these from coordinates: a checkpoint that disagrees was written by another definition
                got = torch.as_tensor(sd[k]).detach().to("cpu")
                if tuple(got.shape) != tuple(want.shape) or not torch.equal(got.to(want.dtype), want):
                    raise RuntimeError(f"buffer {k} of the checkpoint differs from the canonical relative position index of a {self.backbone.window_size}x{self.backbone.window_size} window")
        for k, shape in self.param_shapes.items():
            if k in sd:
                t = torch.as_tensor(sd[k]).detach().to("cpu", torch.float32).contiguous()
                if tuple(t.shape) != tuple(shape):
                    raise RuntimeError(f"size mismatch for {k}: checkpoint {tuple(t.shape)} vs model {tuple(shape)}")
                self._state[k] = t
        if self._live_params is not None:  # a TrainingModule owns the parameters on the device: keep its arena in step
            self._live_params.copy_(self.flat_params())
        self._release()
        return missing, unexpected

    def init_xavier_(self, seed: int = 0, head_scale: float = 1.0) -> "Model":
        """Fresh weights the way the reference's trainer initialises a model (``xavier_init_weights``,
        training/utils.py:72-78): Xavier-uniform Conv2d / Linear weights, zero biases; LayerNorm affine = (1, 0),
        ConvNeXt ``layer_scale`` = 1e-6 (the module defaults).  ``head_scale`` shrinks the head weights (synthetic
        benchmarks keep the raw outputs O(1) that way).  Deterministic in ``seed``."""
        import math

        g = torch.Generator().manual_seed(int(seed))
        sd = {}
        for k, shape in self.param_shapes.items():
            if k.endswith(".layer_scale"):
                sd[k] = torch.full(shape, 1e-6)
            elif len(shape) == 1:
                ln = k.endswith(".weight") and (any(o.kind in (L.OP_LAYERNORM, L.OP_PATCH_MERGE) and o.weight == k for o in self.unfused_ops) or
                                                k in getattr(self.backbone, "unit_init_keys", ()))  # (a ResNet backbone's BatchNorm weights: the module default)
                sd[k] = torch.ones(shape) if ln else torch.zeros(shape)
            else:
                rf = 1
                for d in shape[2:]:
                    rf *= int(d)
                fan_in, fan_out = int(shape[1]) * rf, int(shape[0]) * rf
                bound = math.sqrt(6.0 / (fan_in + fan_out))
                w = (torch.rand(shape, generator=g) * 2 - 1) * bound
                sd[k] = w * head_scale if k.startswith("head_layers.") else w
        sd.update(self.buffers)
        self.load_state_dict(sd, strict=True)
        return self

    def num_parameters(self) -> int:
        return sum(int(torch.tensor(s).prod()) for s in self.param_shapes.values())

    def eval(self) -> "Model":
        return self.set_fusion(True)

    def train(self, mode: bool = True, allow_swint: bool = False, allow_pretrained: bool = False) -> "Model":
        """Training keeps every activation: the op-by-op (unfused) program runs.  A Swin backbone trains on request only
        (``allow_swint=True``; ``TrainingModule(model, swint_training=True)`` passes it): its backward is the window-attention,
        patch-merge and residual steps of ``ph_model_backward`` (csrc/swin_train_kernels.hip).  So does a ``pretrained`` (ConvNeXtV2)
        backbone (``allow_pretrained=True``; ``TrainingModule(model, pretrained_training=True)``): its GRN and stem ops keep ``FLAG_NO_TRAIN`` and the handle
        option ``pretrained_train`` lifts the refusal of ``ph_model_backward`` (csrc/convnextv2_train_kernels.hip).  The training program is the
        unfused one: it runs the two-launch GRN forward whatever ``grn_fuse`` says."""
        if mode and self.is_resnet:
            raise NotImplementedError("a 'pretrained' ResNet backbone is inference only on the MI355X path: its program runs BatchNorm folded into the convs (eval statistics); "
                                      "training needs BatchNorm with batch statistics, which is not built (sleap_nn_amd/architectures/pretrained.py)")
        if mode and self.is_swinv2:
            raise NotImplementedError("a 'pretrained' Swinv2 backbone is inference only on the MI355X path: its cosine window attention, residual-after-norm LayerNorm and "
                                      "norm-less patch merge have no backward step (sleap_nn_amd/architectures/pretrained.py)")
        if mode and self.backbone_type == "pretrained":
            if not allow_pretrained:
                raise NotImplementedError("training a 'pretrained' (ConvNeXtV2) backbone is opt-in on the MI355X path (its GRN and padding-0 stem ops carry PH_FLAG_NO_TRAIN): "
                                          "Model.train(True, allow_pretrained=True), or TrainingModule(model, pretrained_training=True)")
            self.backbone.check_trainable()
            self.set_option("pretrained_train", 1)
        if mode and self.backbone_type == "swint" and not allow_swint:
            raise NotImplementedError("training a 'swint' backbone is opt-in on the MI355X path: Model.train(True, allow_swint=True), or "
                                      "TrainingModule(model, swint_training=True)")
        return self.set_fusion(not mode)

    @property
    def is_resnet(self) -> bool:
        """A ``pretrained`` backbone of the ResNet family (HuggingFace ResNetBackbone): BatchNorm folded at handle creation, exact fp32, inference only."""
        return self.backbone_type == "pretrained" and getattr(self.backbone, "family", "") == "resnet"

    @property
    def is_swinv2(self) -> bool:
        """A ``pretrained`` backbone of the Swinv2 family (HuggingFace Swinv2Backbone): qkv, bias table and logit scales derived at handle creation, exact fp32, inference only."""
        return self.backbone_type == "pretrained" and getattr(self.backbone, "family", "") == "swinv2"

    def trainable_ranges(self, freeze_encoder: Optional[bool] = None) -> List[tuple]:
        """``[(start, end), ...]`` of the flat parameter arena (``param_keys`` order) that an optimizer steps: sorted, disjoint, on parameter boundaries, neighbours
        merged.  Left out are the parameters no op of the program reads (a ``pretrained`` backbone's ``hidden_states_norms.stem``: torch leaves their ``.grad`` at
        ``None`` and its optimizers skip them, so not even AdamW's decay may touch them) and, with ``freeze_encoder`` (default: the backbone config's ``freeze``),
        every ``backbone.enc.*`` parameter -- the reference's ``freeze_encoder()``."""
        freeze = bool(getattr(self.backbone, "freeze", False)) if freeze_encoder is None else bool(freeze_encoder)
        # an op is live when it is a head or a live op reads its output (a stage norm whose map the decoder does not take is an op, and dead: output_stride 8)
        read, live_slots = set(), set()
        for o in reversed(self.unfused_ops):
            if o.kind == L.OP_HEAD or o.dst in live_slots or (o.dst2 >= 0 and o.dst2 in live_slots):
                live_slots.update(s for s in (o.src0, o.src1) if s >= 0)
                read.update(k for k in (o.weight, o.bias, o.weight2, o.bias2) if k)
        out: List[tuple] = []
        off = 0
        for k in self.param_keys():
            n = 1
            for d in self.param_shapes[k]:
                n *= int(d)
            if k in read and not (freeze and k.startswith("backbone.enc.")):
                if out and out[-1][1] == off:
                    out[-1] = (out[-1][0], off + n)
                else:
                    out.append((off, off + n))
            off += n
        return out

    def adapt_channels(self, x: torch.Tensor, code: int):
        """architectures/model.py:239-245 (gray <-> rgb) for a frame whose channel count is not the network's: ``(x, dtype code)`` as the native calls take them.
        Rare path, done with torch plumbing; the result is float in [0, 1] (code 1)."""
        if x.shape[1] == self.in_channels:
            return x, code
        xf = x.float() / 255.0 if code in (0, 2) else x
        if x.shape[1] == 1:
            xf = xf.repeat(1, 3, 1, 1)
        elif x.shape[1] == 3:
            r, g, b = xf.unbind(dim=1)
            xf = (0.2989 * r + 0.587 * g + 0.114 * b).unsqueeze(1)
        return xf, 1

    def residual_branches(self) -> int:
        """Number of residual Linear ops (``FLAG_RESIDUAL``) of the current program: the rows of ``ph_model_set_branch_scales``."""
        return sum(1 for o in self.ops if o.kind == L.OP_LINEAR and (o.flags & L.FLAG_RESIDUAL))

    def last_backward_kernels(self):
        """PH_KV_* code of the kernel each op's step of the LAST ``ph_model_backward`` ran (``ph_model_last_backward_kernels``)."""
        n = len(self.ops)
        arr = (C.c_int32 * n)()
        L.check(L.lib().ph_model_last_backward_kernels(self._handle, arr, n))
        return list(arr)

    def last_backward_routes(self):
        """PH_BR_* route word of each op's step of the LAST ``ph_model_backward`` (``ph_model_last_backward_routes``; ``_lib.br_decode`` names the fields).  0 for an op
        that ran no step (a frozen prefix, an op nobody reads)."""
        n = len(self.ops)
        arr = (C.c_int32 * n)()
        L.check(L.lib().ph_model_last_backward_routes(self._handle, arr, n))
        return list(arr)

    def set_fusion(self, fused: bool) -> "Model":
        want = self.fused_ops if fused else self.unfused_ops
        if want is not self.ops:
            self.ops = want
            self._release()
        # the training program keeps fp32 activations for the backward pass; inference runs at `self.precision` and lets
        # activation slots share memory once their last reader has run (unless somebody wants to read them back)
        self.set_option("conv_precision", PRECISIONS[self.precision] if fused else 0)
        self.set_option("workspace_reuse", 1 if (fused and not self.keep_activations) else 0)
        return self

    def set_keep_activations(self, keep: bool) -> "Model":
        """``True``: every activation of an inference forward stays readable (``read_activation``) at the price of one memory
        range per slot (9.0 instead of 3.6 GB at cfg3 x 32 frames)."""
        self.keep_activations = bool(keep)
        if self.ops is self.fused_ops:
            self.set_option("workspace_reuse", 0 if self.keep_activations else 1)
        return self

    def set_precision(self, precision: str, convnext_f16: Optional[bool] = None, swint_f16: Optional[bool] = None) -> "Model":
        """Arithmetic of the inference forward:
        ``"exact"``: fp32 products on the fp32 matrix pipe (bit-for-bit a k-ordered fmaf chain);
        ``"split"``: every operand as a (hi, lo) pair of fp16 numbers, three fp16 MFMAs per product with fp32 accumulation --
        22-bit products, ~1e-6 relative on the head outputs, 16/3 of the fp32 matrix rate.  UNet programs only: a ConvNeXt
        program set to ``"split"`` runs exact;
        ``"fp16"``: plain fp16 operands and storage, fp32 accumulation -- the reference's autocast mode
        (torch_backend.py:113-143; its tolerance is 5e-3).  UNet programs run their 3x3 convolutions on the fp16 matrix pipe.
        ConvNeXt programs run whole in fp16 storage when the handle option ``convnext_f16`` is 1 as well: patch stem,
        depthwise 7x7 + LayerNorm, both Linear layers of a CNBlock and the 2x2 downsampling convs as fp16 MFMA row GEMMs
        with fp32 accumulators, fp32 LayerNorm moments and fp32 erf-GELU, the residual stream stored in fp16,
        then the fp16 decoder.  ``convnext_f16=True`` / ``False`` sets that option here (``None`` leaves it as it is; a
        ``set_option("convnext_f16", 1)`` before a ``HipBackend(model, use_fp16=True)`` does the same).  It is 0 by default,
        and a ConvNeXt program then runs exact under every precision, as it always did: tests/test_gpu_plan_hazards.py pins the
        fp32 plan of ConvNeXt programs (its one-launch CNBlock MLP included) under ``"split"`` and ``"fp16"``.
        Swin programs have a switch of their own, the handle option ``swint_f16`` (``swint_f16=True`` / ``False`` here, or
        ``set_option("swint_f16", 1)`` before a ``HipBackend(model, use_fp16=True)``; 0 by default, independent of
        ``convnext_f16``): with it ``"fp16"`` runs the whole program in fp16 storage -- patch stem, LayerNorms (fp32 moments),
        the qkv / proj / MLP / reduction Linears as fp16 MFMA row GEMMs with fp32 accumulators and epilogues, window attention
        on the fp16 matrix pipe with fp32 logits and softmax statistics, the patch-merge norm, the residual stream stored in
        fp16, then the fp16 decoder.  Without it a Swin program runs exact under every precision
        (tests/test_gpu_swint.py pins that); ``"split"`` is exact for it either way.
        A ``pretrained`` (ConvNeXtV2) program has no fp16 form: it runs exact under every precision and whatever ``convnext_f16`` says (tests/test_gpu_pretrained.py);
        so does a ``pretrained`` ResNet program (tests/test_gpu_pretrained_resnet.py) and a ``pretrained`` Swinv2 program, whatever ``swint_f16`` says
        (tests/test_gpu_pretrained_swinv2.py).
        Programs with a class-vector head (global max pool, softmax) and every training program run exact whatever is set."""
        if precision not in PRECISIONS:
            raise ValueError(f"precision must be one of {sorted(PRECISIONS)}, got {precision!r}")
        self.precision = precision
        if convnext_f16 is not None:
            self.set_option("convnext_f16", 1 if convnext_f16 else 0)
        if swint_f16 is not None:
            self.set_option("swint_f16", 1 if swint_f16 else 0)
        if self.ops is self.fused_ops:
            self.set_option("conv_precision", PRECISIONS[precision])
        return self

    def param_keys(self) -> List[str]:
        """Order of the canonical flat parameter arena (= ph_model_create's weights[])."""
        return list(self.param_shapes.keys())

    def flat_params(self) -> torch.Tensor:
        return torch.cat([self._state[k].reshape(-1) for k in self.param_keys()])

    def load_flat_params(self, flat: torch.Tensor) -> None:
        """Host copy of the arena back into the state dict (e.g. for checkpointing)."""
        flat = flat.detach().to("cpu", torch.float32)
        o = 0
        for k in self.param_keys():
            n = self._state[k].numel()
            self._state[k] = flat[o : o + n].reshape(self.param_shapes[k]).clone()
            o += n

    def to(self, device) -> "Model":
        self.device = torch.device(device)
        return self

    # -- native handle ----------------------------------------------------------------------
    def _release(self) -> None:
        if self._handle is not None:
            L.lib().ph_model_destroy(self._handle)
            self._handle = None
            self.generation += 1

    def set_option(self, key: str, value: float) -> "Model":
        """Per-handle kernel-variant option (``ph_model_set_option``; keys in include/posehip.h).  Remembered across recompiles."""
        if self._handle is not None:
            L.check(L.lib().ph_model_set_option(self._handle, str(key).encode(), float(value)))
        if self._options.get(str(key)) != float(value):
            self.generation += 1  # a captured hipGraph replays the kernels it was captured with: stale after a variant change
        self._options[str(key)] = float(value)
        return self

    def set_head_loss(self, index: int, kind: int, params=()) -> "Model":
        """Loss of head ``index`` in ``ph_model_backward`` (``ph_model_set_head_loss``; kinds ``_lib.LOSS_*``).  Remembered across recompiles, like the
        options, and applied to the handle of the training (unfused) program only: with ``LOSS_BCE_DICE`` that program's head emits logits, while the
        inference program keeps returning probabilities."""
        self._head_losses[int(index)] = (int(kind), tuple(float(p) for p in params))
        if self._handle is not None and self.ops is self.unfused_ops:
            self._apply_head_losses()
            self.generation += 1
        return self

    def _apply_head_losses(self) -> None:
        for i, (kind, params) in self._head_losses.items():
            arr = (C.c_float * max(1, len(params)))(*params)
            L.check(L.lib().ph_model_set_head_loss(self._handle, i, kind, arr, len(params)))

    def get_option(self, key: str) -> float:
        if self._handle is None:
            raise RuntimeError("get_option needs a compiled handle (run a forward first)")
        v = C.c_double()
        L.check(L.lib().ph_model_get_option(self._handle, str(key).encode(), C.byref(v)))
        return v.value

    def bind_live_params(self, flat_dev: Optional[torch.Tensor]) -> None:
        """Device arena (canonical order) that owns the live parameters, or None to go back to the host state dict."""
        self._live_params = flat_dev

    def __del__(self):
        try:
            self._release()
        except Exception:
            pass

    def _compile(self, device: torch.device) -> None:
        lib = L.lib()
        keys = list(self.param_shapes.keys())
        index = {k: i for i, k in enumerate(keys)}
        descs = (L.OpDesc * len(self.ops))()
        for i, op in enumerate(self.ops):
            d = descs[i]
            d.kind, d.src0, d.src1, d.dst = op.kind, op.src0, op.src1, op.dst
            d.cin0, d.cin1, d.cout, d.ksize, d.flags = op.cin0, op.cin1, op.cout, op.ksize, op.flags
            d.weight = index[op.weight] if op.weight else -1
            d.bias = index[op.bias] if op.bias else -1
            d.out_index = op.out_index
            d.dst2, d.cmid = op.dst2, op.cmid
            d.weight2 = index[op.weight2] if op.weight2 else -1
            d.bias2 = index[op.bias2] if op.bias2 else -1
        # a ResNet backbone: the conv ops read W * g / sqrt(var + eps) and beta - mean * g / sqrt(var + eps) where the arena has W and beta -- folded here, from the state and
        # the buffers as they stand (load_state_dict releases the handle, so a fold never outlives what it was made from); _state keeps the unfolded tensors
        # a Swinv2 backbone: the qkv Linear and the attention op read the concatenated query | key | value, the padded token's q | 0 | v, the 16 sigmoid(MLP) bias table and the
        # clamped, exponentiated logit scales under four of each block's keys (derived_params), by the same mechanism
        folded = self.backbone.folded_params(self._state, self.buffers) if self.is_resnet else self.backbone.derived_params(self._state, self.buffers) if self.is_swinv2 else {}
        tensors = [folded.get(k, self._state[k]).contiguous() for k in keys]
        ptrs = (C.c_void_p * len(keys))(*[t.data_ptr() for t in tensors])
        numel = (C.c_int64 * len(keys))(*[t.numel() for t in tensors])
        with torch.cuda.device(device):
            h = lib.ph_model_create(descs, len(self.ops), ptrs, numel, len(keys), self.backbone.n_slots, len(self.heads))
        if not h:
            raise L.PosehipError(L.PH_E_INVALID, lib.ph_last_error().decode())
        self._handle = C.c_void_p(h)
        self._handle_device = device
        self.generation += 1
        for k, v in self._options.items():
            L.check(lib.ph_model_set_option(self._handle, k.encode(), v))
        if self._loaded_buffers:  # input statistics of the padding-0 patch stem
            mean = [float(v) for v in self.buffers["backbone.image_mean"].reshape(-1)]
            std = [float(v) for v in self.buffers["backbone.image_std"].reshape(-1)]
            L.check(lib.ph_model_set_input_norm(self._handle, (C.c_float * len(mean))(*mean), (C.c_float * len(std))(*std), len(mean)))
        if self.ops is self.unfused_ops:
            self._apply_head_losses()
        if self._live_params is not None:  # the host copy in _state may be stale during training
            if self._live_params.device != device or self._live_params.numel() != sum(t.numel() for t in tensors):
                raise RuntimeError("live parameter arena does not match this model / device")
            with torch.cuda.device(device):
                L.check(lib.ph_model_set_params(self._handle, C.c_void_p(self._live_params.data_ptr()), L.current_stream_ptr()))

    def _ensure(self, device: torch.device) -> None:
        if self._handle is None or self._handle_device != device:
            self._release()
            self._compile(device)

    def output_shapes(self, height: int, width: int):
        lib = L.lib()
        out = []
        for i in range(len(self.heads)):
            c, h, w = C.c_int32(), C.c_int32(), C.c_int32()
            L.check(lib.ph_model_output_shape(self._handle, i, height, width, C.byref(c), C.byref(h), C.byref(w)))
            out.append((c.value, h.value, w.value))
        return out

    # -- forward --------------------------------------------------------------------------
    def forward(self, x: torch.Tensor, in_dtype: Optional[int] = None) -> Dict[str, torch.Tensor]:
        """``x``: (B, C, H, W) on the GPU.  uint8 is divided by 255 inside the first kernel;
        float input is taken as already normalised unless ``in_dtype == 2`` (0..255 floats)."""
        if x.dim() != 4:
            raise ValueError(f"expected (B, C, H, W), got {tuple(x.shape)}")
        if not x.is_cuda:
            dev = self.device if self.device.type == "cuda" else torch.device("cuda", torch.cuda.current_device())
            x = x.to(dev, non_blocking=True)
        device = x.device
        if x.dtype == torch.uint8:
            code = 0
        else:
            x = x.to(torch.float32)
            code = 1 if in_dtype is None else in_dtype
        x, code = self.adapt_channels(x, code)
        x = x.contiguous()
        B, Cin, H, W = x.shape
        if (self.is_resnet or self.is_swinv2) and (H % self.backbone.max_stride or W % self.backbone.max_stride):  # every strided conv / patch merge must see an even map: anything else would be another network's map
            raise ValueError(f"a 'pretrained' {'ResNet' if self.is_resnet else 'Swinv2'} backbone takes frames whose height and width are multiples of {self.backbone.max_stride}, got {H} x {W} "
                             "(the inference layers pad to max_stride)")
        self._last_batch = int(B)
        self._ensure(device)
        lib = L.lib()
        with torch.cuda.device(device):
            need = L.check(lib.ph_model_workspace_bytes(self._handle, B, H, W))
            if self._workspace is None or self._workspace.numel() < need or self._workspace.device != device:
                self._workspace = None
                self._workspace = torch.empty(int(need), dtype=torch.uint8, device=device)
                self.generation += 1
            outs = [torch.empty((B, c, h, w), dtype=torch.float32, device=device) for (c, h, w) in self.output_shapes(H, W)]
            optrs = (C.c_void_p * len(outs))(*[o.data_ptr() for o in outs])
            L.check(
                lib.ph_model_forward(
                    self._handle, C.c_void_p(x.data_ptr()), code, B, Cin, H, W, C.c_void_p(self._workspace.data_ptr()),
                    self._workspace.numel(), optrs, L.current_stream_ptr(),
                )
            )
        return {head.name: (o.flatten(1) if isinstance(head, ClassVectorsHead) else o) for head, o in zip(self.heads, outs)}

    __call__ = forward

    # -- measurement support ------------------------------------------------------------
    def set_profiling(self, enabled, resume: bool = False) -> None:
        """Per-op HIP-event timing on the forward's stream (bench.py roofline).  ``resume=True`` switches recording back on
        without clearing what was accumulated (sampling every n-th forward of a timed region)."""
        L.check(L.lib().ph_model_set_profiling(self._handle, (2 if resume else 1) if enabled else 0))

    def read_profile(self):
        """-> (list of accumulated ms per op, number of forwards covered)."""
        n = len(self.ops)
        arr = (C.c_double * n)()
        k = C.c_int32()
        L.check(L.lib().ph_model_profile_read(self._handle, arr, n, C.byref(k)))
        return list(arr), k.value

    def last_kernels(self):
        """PH_KV_* code (``_lib.KV_*``) of the kernel family each op of the LAST forward ran; the library's own record of
        its dispatch (``ph_model_last_kernels``), so FLOP accounting never restates the dispatch rules."""
        n = len(self.ops)
        arr = (C.c_int32 * n)()
        L.check(L.lib().ph_model_last_kernels(self._handle, arr, n))
        return list(arr)

    def last_rows_plans(self):
        """``(R, Wt, MT, MG)`` of each op of the LAST forward that ran ``conv3x3_f16_rows_kernel`` (``ph_model_last_rows_plans``), ``(0, 0, 0, 0)`` for an op on any other
        kernel.  The kernel instantiation is ``(Wt % 16 == 0, MT, MG)``; the handle option ``conv_f16_rows_pin`` (``R | Wt << 8 | MG << 16``) pins the tile."""
        n = len(self.ops)
        arr = (C.c_int32 * (4 * n))()
        L.check(L.lib().ph_model_last_rows_plans(self._handle, arr, n))
        return [tuple(arr[4 * i : 4 * i + 4]) for i in range(n)]

    def last_ranges(self):
        """Workspace byte ranges every launch of the LAST forward was handed (``ph_model_last_ranges``), as the run-time routing
        decided them: a list of ``(op index, launch ordinal within the op, is_dst, slot, byte offset, bytes)``.  An op without a
        launch of its own has no entry; the scratch region behind the slots (slot -1) counts as a destination of the launches that
        use it."""
        n = C.c_int32()
        L.check(L.lib().ph_model_last_ranges(self._handle, None, 0, C.byref(n)))
        arr = (C.c_int64 * (6 * max(1, n.value)))()
        L.check(L.lib().ph_model_last_ranges(self._handle, arr, n.value, C.byref(n)))
        return [(int(arr[6 * i]), int(arr[6 * i + 1]), bool(arr[6 * i + 2]), int(arr[6 * i + 3]), int(arr[6 * i + 4]), int(arr[6 * i + 5])) for i in range(n.value)]

    def debug_allocs(self, read_first: int = 0):
        """Every device allocation the handle owns, in the order it was made (``ph_model_debug_allocs``): a list of ``(pointer, bytes)``.  With
        ``read_first = n`` the list is cut to the first ``n`` allocations and each entry is a host ``uint8`` tensor of the allocation's bytes instead
        (the device is synchronised first)."""
        lib = L.lib()
        n = C.c_int32()
        L.check(lib.ph_model_debug_allocs(self._handle, None, None, 0, C.byref(n)))
        ptrs, sizes = (C.c_void_p * max(1, n.value))(), (C.c_int64 * max(1, n.value))()
        L.check(lib.ph_model_debug_allocs(self._handle, ptrs, sizes, n.value, C.byref(n)))
        rows = [(int(ptrs[i] or 0), int(sizes[i])) for i in range(n.value)]
        if not read_first:
            return rows
        torch.cuda.synchronize()
        out = []
        for ptr, size in rows[:read_first]:
            host = torch.empty(size, dtype=torch.uint8)
            rc = lib.hipMemcpy(C.c_void_p(host.data_ptr()), C.c_void_p(ptr), C.c_size_t(size), 2)  # (hipMemcpyDeviceToHost; the runtime libposehip is linked against)
            if rc != 0:
                raise RuntimeError(f"hipMemcpy of allocation {len(out)} ({size} bytes) failed with {rc}")
            out.append(host)
        return out

    def op_table(self, batch: int, height: int, width: int):
        """Per op: label, kind, algorithmic FLOPs (2*Cin*Cout*k*k*Hout*Wout*B for convolutions, SURVEY
        section 8d) and algorithmic HBM bytes (input read once + output written once, logical channels)."""
        hw = {-1: (height, width)}
        ch = {-1: self.in_channels}
        rows = []
        for op in self.ops:
            h, w = hw[op.src0]
            if op.kind == L.OP_STEM:
                f0 = 2.0 * op.cin0 * op.cmid * 9 * h * w * batch
                f1 = 2.0 * op.cmid * op.cout * 9 * h * w * batch
                ph, pw = (h + 1) // 2, (w + 1) // 2
                byt = op.cin0 * h * w * batch + 4 * op.cout * ph * pw * batch + (4 * op.cout * h * w * batch if op.dst >= 0 else 0)
                rows.append({"label": op.label.split(".")[-1], "kind": op.kind, "flops": f0 + f1, "mfma_flops": f1, "bytes": float(byt)})
                if op.dst >= 0:
                    hw[op.dst] = (h, w)
                hw[op.dst2] = (ph, pw)
                continue
            if op.kind == L.OP_RESNET_STEM:
                fh, fw = (h - 1) // 2 + 1, (w - 1) // 2 + 1
                hw[op.dst], hw[op.dst2] = (fh, fw), ((fh - 1) // 2 + 1, (fw - 1) // 2 + 1)
                rows.append({"label": op.label.split(".")[-1], "kind": op.kind, "flops": 2.0 * op.cin0 * op.cout * 49 * fh * fw * batch,
                             "bytes": float(op.cin0 * h * w * batch + 4 * op.cout * (2 * fh * fw + hw[op.dst2][0] * hw[op.dst2][1]) * batch),
                             "cin0": op.cin0, "cin1": 0, "cout": op.cout, "ksize": 7, "out_hw": hw[op.dst2]})
                continue
            oh, ow = h, w
            if op.kind == L.OP_CONV_S2:
                oh, ow = h // 2, w // 2
            if op.kind == L.OP_PATCH_STEM:
                pad2 = 0 if op.flags & L.FLAG_PAD0_NORM else 2
                oh, ow = (h + pad2 - op.ksize) // op.cmid + 1, (w + pad2 - op.ksize) // op.cmid + 1
            elif op.kind == L.OP_PATCH_CONV:
                oh, ow = h // 2, w // 2
            elif op.kind == L.OP_PATCH_MERGE:
                oh, ow = (h + 1) // 2, (w + 1) // 2
            if op.kind in (L.OP_WINDOW_ATTN, L.OP_WINDOW_ATTN_V2):
                # q k^T and p v: 2 * N * d multiply-adds each per token and head (cin1 = heads, ksize = window side, head dimension cout / heads)
                rows.append({"label": op.label.split(".")[-1], "kind": op.kind, "flops": 4.0 * op.ksize * op.ksize * op.cout * h * w * batch,
                             "bytes": float(4 * (op.cin0 + op.cout) * h * w * batch), "cin0": op.cin0, "cin1": 0, "cout": op.cout, "ksize": op.ksize, "out_hw": (h, w)})
                hw[op.dst] = (h, w)
                continue
            if op.kind == L.OP_POOL:
                oh, ow = (h + 1) // 2, (w + 1) // 2
            elif op.kind in (L.OP_UPSAMPLE, L.OP_CONVT):
                oh, ow = 2 * h, 2 * w
            cin = op.cin0 + (op.cin1 if op.kind not in (L.OP_LINEAR, L.OP_SCALE_ADD, L.OP_ADD_RELU) else 0)
            cout = op.cout if op.kind not in (L.OP_POOL, L.OP_UPSAMPLE) else op.cin0
            flops = 0.0
            if op.kind in (L.OP_CONV, L.OP_INPUT_CONV, L.OP_CONV_S2):
                flops = 2.0 * cin * cout * op.ksize * op.ksize * oh * ow * batch
            elif op.kind == L.OP_CONVT:
                flops = 2.0 * cin * cout * 9 * h * w * batch
            elif op.kind in (L.OP_HEAD, L.OP_LINEAR):
                flops = 2.0 * cin * cout * oh * ow * batch
            elif op.kind in (L.OP_PATCH_STEM, L.OP_PATCH_CONV):
                flops = 2.0 * cin * cout * op.ksize * op.ksize * oh * ow * batch
            elif op.kind == L.OP_DWCONV:
                flops = 2.0 * cout * 49 * oh * ow * batch
            in_bytes = (1 if op.src0 < 0 else 4) * op.cin0 * h * w * batch + 4 * op.cin1 * h * w * batch
            out_bytes = 4 * cout * oh * ow * batch
            rows.append({"label": op.label.split(".")[-1], "kind": op.kind, "flops": flops, "bytes": float(in_bytes + out_bytes),
                         "cin0": op.cin0, "cin1": op.cin1, "cout": cout, "ksize": op.ksize, "out_hw": (oh, ow)})
            if op.kind != L.OP_HEAD:
                hw[op.dst] = (oh, ow)
            if op.kind == L.OP_CONV and op.dst2 >= 0:
                hw[op.dst2] = ((oh + 1) // 2, (ow + 1) // 2)
        return rows

    def read_activation(self, conv_name: str, batch: int, height_width) -> torch.Tensor:
        """Debug/parity: NCHW copy of the activation a named conv produced in the last forward."""
        if self.ops is self.fused_ops and not self.keep_activations:
            raise RuntimeError("activation slots are recycled during an inference forward: call set_keep_activations(True) before the forward")
        slot = self.backbone.labels[conv_name]
        op = next((o for o in self.ops if o.dst == slot), None)
        if op is None:
            raise KeyError(f"activation of {conv_name} is fused away (it never exists in HBM)")
        h, w = height_width
        out = torch.empty((batch, op.cout, h, w), dtype=torch.float32, device=self._handle_device)
        L.check(L.lib().ph_model_read_slot(self._handle, slot, C.c_void_p(out.data_ptr()), out.numel(), L.current_stream_ptr()))
        return out

    def read_slot(self, slot: int, channels: int, height_width) -> torch.Tensor:
        """Debug/parity: NCHW copy of activation slot ``slot`` of the last forward (``ph_model_read_slot``) -- any tensor of a keep-everything plan, pool outputs and
        up-sampled tensors included, where ``read_activation`` reaches the named convs.  The batch is the last forward's."""
        if self.ops is self.fused_ops and not self.keep_activations and self._options.get("workspace_reuse", 1.0) == 1.0:
            raise RuntimeError("activation slots are recycled during an inference forward: call set_keep_activations(True) before the forward")
        h, w = height_width
        out = torch.empty((self._last_batch, int(channels), h, w), dtype=torch.float32, device=self._handle_device)
        L.check(L.lib().ph_model_read_slot(self._handle, int(slot), C.c_void_p(out.data_ptr()), out.numel(), L.current_stream_ptr()))
        return out
