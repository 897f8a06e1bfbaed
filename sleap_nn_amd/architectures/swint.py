"""Swin Transformer encoder + UNet-style decoder -> op program for libposehip (inference and, on request, training).

Reproduces the structure and the checkpoint parameter names of the reference ``SwinTWrapper``
(``sleap_nn/architectures/swint.py:41-163`` encoder, ``:166-400`` wrapper) without torch modules.  The encoder
blocks are torchvision's (``SwinTransformerBlock`` / ``ShiftedWindowAttention`` / ``PatchMerging``, version 1);
their state_dict layout is kept (``features.{i}.{j}.{norm1,attn.qkv,attn.proj,attn.relative_position_bias_table,
norm2,mlp.0,mlp.3}``, ``features.{i}.{norm,reduction}``, ``enc.norm``) so reference checkpoints load;
``attn.relative_position_index`` is a buffer: checked against the canonical index at load, never a parameter.

In the NHWC layout of the kernels a block is seven launches: LayerNorm -> row GEMM C->3C (qkv, on the un-padded,
un-rolled map) -> window attention (pad, roll, partition, bias, band mask, softmax, reverse and crop in one
kernel) -> row GEMM C->C whose epilogue adds the block input -> LayerNorm -> row GEMM C->4C with the erf-GELU in
its epilogue -> row GEMM 4C->C whose epilogue adds the residual.  Patch merging is the four-phase gather with its
LayerNorm in one launch, then a bias-less row GEMM.  All norms have eps 1e-5.  Dropout is 0 in the reference; stochastic
depth is the identity at inference.  Training is opt-in (``Model.train(True, allow_swint=True)``,
``TrainingModule(model, swint_training=True)``): the op-by-op program keeps the qkv slot, the attention output, both
LayerNorm inputs and the GELU input, and ``ph_model_backward`` runs the attention core's backward
(``csrc/swin_train_kernels.hip``: S and P recomputed, fixed-order reductions), the patch-merge backward
and the residual fan-out.  Stochastic depth -- the reference builds its encoder with torchvision's default
``stochastic_depth_prob = 0.1`` (swint.py:80, :117-133) -- is a per-sample scale of each residual branch, drawn by
``draw_branch_scales`` and handed to the library with ``ph_model_set_branch_scales``.  The same program runs in exact fp32 (the default) or,
with ``Model.set_precision("fp16", swint_f16=True)``, whole on fp16 activations (``csrc/swin_f16_kernels.hip``).

The pool / middle / decoder half is the ConvNeXt wrapper's, as in the reference (swint.py:266-339).
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Dict, List, Tuple

import torch

from sleap_nn_amd import _lib as L
from sleap_nn_amd.architectures.convnext import ConvNextWrapper
from sleap_nn_amd.architectures.unet import OpSpec
from sleap_nn_amd.utils import cfg_get

ARCH_TYPES = {
    # swint.py:225-237
    "tiny": {"embed": 96, "depths": [2, 2, 6, 2], "num_heads": [3, 6, 12, 24]},
    "small": {"embed": 96, "depths": [2, 2, 18, 2], "num_heads": [3, 6, 12, 24]},
    "base": {"embed": 128, "depths": [2, 2, 18, 2], "num_heads": [4, 8, 16, 32]},
}
HEAD_DIM = 32  # what window_attn_kernel is built for
LN = L.FLAG_LN_EPS_1EM5


def relative_position_index(window: int) -> torch.Tensor:
    """torchvision's ``_get_relative_position_index`` for a square window: int64 (window^4,)."""
    coords = torch.stack(torch.meshgrid(torch.arange(window), torch.arange(window), indexing="ij")).flatten(1)
    rel = (coords[:, :, None] - coords[:, None, :]).permute(1, 2, 0).contiguous()
    rel[:, :, 0] += window - 1
    rel[:, :, 1] += window - 1
    rel[:, :, 0] *= 2 * window - 1
    return rel.sum(-1).flatten()


def stochastic_depth_probs(depths, stochastic_depth_prob: float = 0.1) -> List[float]:
    """Drop probability of block k (over all stages, in order): ``stochastic_depth_prob * k / (total_blocks - 1)`` (swint.py:110-137, torchvision's schedule)."""
    total = int(sum(depths))
    return [float(stochastic_depth_prob) * float(k) / (total - 1) for k in range(total)]


def draw_branch_scales(depths, batch: int, stochastic_depth_prob: float = 0.1, generator=None, device="cpu") -> torch.Tensor:
    """``(2 * sum(depths), batch)`` fp32 scales of the residual branches in program order (attention branch, then MLP branch, of each block):
    ``bernoulli(1 - p_k) / (1 - p_k)`` per sample, what torchvision's ``StochasticDepth(p_k, "row")`` multiplies a branch by in train mode.  Both
    branches of a block share p_k and are drawn independently."""
    p = torch.tensor(stochastic_depth_probs(depths, stochastic_depth_prob), dtype=torch.float32, device=device).repeat_interleave(2)
    keep = (1.0 - p)[:, None].expand(-1, int(batch))
    drawn = torch.bernoulli(keep, generator=generator)
    return (drawn / keep).contiguous()


@dataclass
class SwinTWrapper(ConvNextWrapper):
    """Config-derived description; ``from_config`` mirrors swint.py:353-374."""

    embed: int = 96
    num_heads: List[int] = field(default_factory=lambda: [3, 6, 12, 24])
    window_size: int = 7
    buffers: Dict[str, torch.Tensor] = field(default_factory=dict)  # non-parameter checkpoint entries (relative_position_index)

    @classmethod
    def from_config(cls, config) -> "SwinTWrapper":
        mt = cfg_get(config, "model_type", None)
        arch = cfg_get(config, "arch", None)
        if mt in ARCH_TYPES:
            a = ARCH_TYPES[mt]
        elif arch is not None:
            a = {"embed": cfg_get(arch, "embed"), "depths": list(cfg_get(arch, "depths")), "num_heads": list(cfg_get(arch, "num_heads"))}
        else:
            a = ARCH_TYPES["tiny"]
        embed = int(a["embed"])
        depths = [int(d) for d in a["depths"]]
        ws = cfg_get(config, "window_size", 7)
        ps = cfg_get(config, "patch_size", 4)
        net = cls(
            model_type=mt,
            output_stride=int(cfg_get(config, "output_stride")),
            depths=depths,
            channels=[embed * 2**i for i in range(len(depths))],
            in_channels=int(cfg_get(config, "in_channels", 1)),
            kernel_size=int(cfg_get(config, "kernel_size", 3)),
            stem_patch_kernel=int(ps[0] if isinstance(ps, (list, tuple)) else ps),
            stem_patch_stride=int(cfg_get(config, "stem_patch_stride", 2)),
            filters_rate=cfg_get(config, "filters_rate", 2),
            convs_per_block=int(cfg_get(config, "convs_per_block", 2)),
            up_interpolate=bool(cfg_get(config, "up_interpolate", True)),
            block_contraction=bool(cfg_get(config, "block_contraction", False)),
            embed=embed,
            num_heads=[int(h) for h in a["num_heads"]],
            window_size=int(ws[0] if isinstance(ws, (list, tuple)) else ws),
        )
        net._build()
        return net

    # -- program construction ---------------------------------------------------------
    def _norm(self, name: str, src: int, c: int) -> int:
        self.param_shapes[name + ".weight"] = (c,)
        self.param_shapes[name + ".bias"] = (c,)
        return self._emit(OpSpec(L.OP_LAYERNORM, src, -1, self._new_slot(), c, 0, c, 1, LN, name + ".weight", name + ".bias", label=name))

    def _linear(self, name: str, src: int, cin: int, cout: int, flags: int = 0, residual: int = -1, bias: bool = True) -> int:
        self.param_shapes[name + ".weight"] = (cout, cin)
        if bias:
            self.param_shapes[name + ".bias"] = (cout,)
        return self._emit(OpSpec(L.OP_LINEAR, src, residual, self._new_slot(), cin, 0, cout, 1, flags, name + ".weight", name + ".bias" if bias else None, label=name))

    def _swin_block(self, name: str, x: int, c: int, heads: int, shift: int) -> int:
        w = self.window_size
        y = self._norm(name + ".norm1", x, c)
        y = self._linear(name + ".attn.qkv", y, c, 3 * c)
        # declared after qkv and before proj: the order torchvision registers them in (parameter arena = state_dict order)
        self.param_shapes[name + ".attn.relative_position_bias_table"] = ((2 * w - 1) ** 2, heads)
        self.buffers[name + ".attn.relative_position_index"] = relative_position_index(w)
        y = self._emit(OpSpec(L.OP_WINDOW_ATTN, y, -1, self._new_slot(), 3 * c, heads, c, w, 0, name + ".attn.relative_position_bias_table", name + ".attn.qkv.bias",
                              label=name + ".attn.core", cmid=shift))
        x = self._linear(name + ".attn.proj", y, c, c, flags=L.FLAG_RESIDUAL, residual=x)
        self.labels[name + ".attn"] = x  # x + attn(norm1(x))
        y = self._norm(name + ".norm2", x, c)
        y = self._linear(name + ".mlp.0", y, c, 4 * c)
        y = self._emit(OpSpec(L.OP_GELU, y, -1, self._new_slot(), 4 * c, 0, 4 * c, 1, 0, label=name + ".mlp.1"))  # (Model folds it into the GEMM's epilogue)
        x = self._linear(name + ".mlp.3", y, 4 * c, c, flags=L.FLAG_RESIDUAL, residual=x)
        self.labels[name] = x
        return x

    def _build(self) -> None:
        if self.kernel_size != 3:
            raise ValueError("only kernel_size=3 is supported by the MFMA convolution kernels")
        if self.block_contraction:
            raise ValueError("block_contraction=True is not supported by the MI355X hot path yet")
        if self.stem_patch_stride not in (1, 2, 4) or not (2 <= self.stem_patch_kernel <= 8) or self.stem_patch_stride > self.stem_patch_kernel:
            raise ValueError("stem_patch_stride must be 1, 2 or 4 and patch_size in 2..8")
        if not (2 <= self.window_size <= 8):
            raise ValueError(f"window_size must be in 2..8 (at most 64 tokens per window), got {self.window_size}")
        if len(self.depths) != 4 or len(self.num_heads) != 4:
            raise ValueError("arch needs four stages: depths and num_heads of length 4")
        ch = self.channels
        for c, h in zip(ch, self.num_heads):
            if h < 1 or c != h * HEAD_DIM:
                raise ValueError(f"num_heads: the head dimension embed * 2^i / num_heads[i] must be {HEAD_DIM}, got {c} channels over {h} heads")
        pfx = "backbone.enc.features"
        # stem: conv k/s, padding 1 -> channel-last -> LayerNorm (features.0.{0,2})
        self.param_shapes[f"{pfx}.0.0.weight"] = (ch[0], self.in_channels, self.stem_patch_kernel, self.stem_patch_kernel)
        self.param_shapes[f"{pfx}.0.0.bias"] = (ch[0],)
        x = self._emit(OpSpec(L.OP_PATCH_STEM, -1, -1, self._new_slot(), self.in_channels, 0, ch[0], self.stem_patch_kernel, 0, f"{pfx}.0.0.weight",
                              f"{pfx}.0.0.bias", label=f"{pfx}.0.0", cmid=self.stem_patch_stride))
        x = self._norm(f"{pfx}.0.2", x, ch[0])
        self.labels[f"{pfx}.0"] = x
        skips: List[Tuple[int, int]] = [(x, ch[0])]  # enc_output[::2]: stem and patch-merging outputs
        fi = 1
        for si, (depth, c) in enumerate(zip(self.depths, ch)):
            for j in range(depth):
                x = self._swin_block(f"{pfx}.{fi}.{j}", x, c, self.num_heads[si], 0 if j % 2 == 0 else self.window_size // 2)
            fi += 1
            if si + 1 < len(ch):
                name = f"{pfx}.{fi}"
                # torchvision registers reduction before norm
                self.param_shapes[name + ".reduction.weight"] = (2 * c, 4 * c)
                self.param_shapes[name + ".norm.weight"] = (4 * c,)
                self.param_shapes[name + ".norm.bias"] = (4 * c,)
                y = self._emit(OpSpec(L.OP_PATCH_MERGE, x, -1, self._new_slot(), c, 0, 4 * c, 2, LN, name + ".norm.weight", name + ".norm.bias", label=name + ".norm"))
                x = self._emit(OpSpec(L.OP_LINEAR, y, -1, self._new_slot(), 4 * c, 0, 2 * c, 1, 0, name + ".reduction.weight", None, label=name + ".reduction"))
                self.labels[name] = x
                skips.append((x, 2 * c))
                fi += 1
        x = self._norm("backbone.enc.norm", x, ch[-1])
        self.labels["backbone.enc.norm"] = x
        self._build_tail(x, skips)
