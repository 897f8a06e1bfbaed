"""HuggingFace ConvNeXtV2 (or, opt-in, ResNet or Swinv2) encoder + UNet-style decoder -> op program for libposehip.

Reproduces Case A (``mode="decoder"``) of the reference ``PretrainedBackbone``
(``sleap_nn/architectures/pretrained.py:111-502``) for the ConvNeXtV2 family, without torch modules and
without ``transformers``: the encoder is HuggingFace's ``ConvNextV2Backbone`` restated as ops, the checkpoint
parameter names are the reference's (``backbone.enc.embeddings...``, ``backbone.enc.encoder.stages.{i}...``,
``backbone.enc.hidden_states_norms.{stem,stage1..4}``, ``backbone.dec.decoder_stack.{b}.blocks.pretrained_dec...``)
and the buffers ``backbone.image_mean`` / ``backbone.image_std`` are read from the checkpoint.

Nothing here can reach a network: the architecture comes from a local directory with a ``config.json`` or from the
size word of a ``convnextv2-<size>`` id; the weights come from the checkpoint.  Every other family, the encoder-only
mode and a subset of the stages are refused by name.

Training is opt-in (``Model.train(True, allow_pretrained=True)``, ``TrainingModule(model, pretrained_training=True)``): the GRN and stem ops
carry ``FLAG_NO_TRAIN``, which ``ph_model_backward`` honours unless the handle option ``pretrained_train`` is set; their backward steps are
``csrc/convnextv2_train_kernels.hip`` and the normalised-patch weight gradient of ``csrc/convnext_train_kernels.hip``.  ``freeze: true``
has the reference's meaning (``freeze_encoder()``, lightning_modules.py:232-236): no ``backbone.enc.*`` parameter receives a gradient or an optimizer
update (``encoder_ops`` / ``Model.trainable_ranges``).  ``drop_path_rate`` of a local ``config.json`` is read and, where non-zero, refused at the opt-in:
the published ConvNeXtV2 configs have 0.0.

The ResNet family (HuggingFace ``ResNetBackbone``; basic and bottleneck layers) is opt-in through the backbone-config key ``allow_resnet`` -- existing tests pin its refusal -- and
inference only: BatchNorm (eval) is folded into each conv on the host (``fold_batchnorm`` / ``folded_params``, float64, at handle creation) while the state dict keeps the
reference's unfolded names; the stem, the strided convs and the residual tails are ``csrc/resnet_kernels.hip`` and the row GEMM's modes 4 and 6.

The Swinv2 family (HuggingFace ``Swinv2Backbone``; effective windows of 2..8, and of 9..24 with ``allow_swinv2_wide`` on top; head dimension 32) is opt-in through the backbone-config key ``allow_swinv2`` for the same reason, and
inference only: per-stage window and shift follow the config's ``image_size`` (``swinv2_windows``); the qkv concatenation, the padded token's q | 0 | v, the ``16 sigmoid(MLP(coords))`` bias
table and the clamped, exponentiated logit scales are derived on the host (``derived_params``, float64, at handle creation) while the state dict keeps the reference's names; the cosine window
attention runs the cosine variant of ``csrc/swin_kernels.hip``'s kernel (key-tiled above window 8: ``csrc/swinv2_kernels.hip``, with the residual-after-norm LayerNorm).

A ConvNeXtV2 block is six ops: depthwise 7x7 -> LayerNorm -> Linear C->4C -> GELU -> GRN -> Linear 4C->C with the residual add
in its epilogue (no layer scale).  ``Model._fuse_cnblocks`` folds the GELU into the first Linear for inference.
"""
from __future__ import annotations

import json
import math
import os
import re
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Tuple

import torch

from sleap_nn_amd import _lib as L
from sleap_nn_amd.architectures.unet import OpSpec
from sleap_nn_amd.utils import cfg_get

THIS_FILE = "sleap_nn_amd/architectures/pretrained.py"

# depths / hidden sizes of the published ConvNeXtV2 sizes (the config.json of facebook/convnextv2-<size>-*)
CONVNEXTV2_SIZES = {
    "atto": {"depths": [2, 2, 6, 2], "hidden_sizes": [40, 80, 160, 320]},
    "femto": {"depths": [2, 2, 6, 2], "hidden_sizes": [48, 96, 192, 384]},
    "pico": {"depths": [2, 2, 6, 2], "hidden_sizes": [64, 128, 256, 512]},
    "nano": {"depths": [2, 2, 8, 2], "hidden_sizes": [80, 160, 320, 640]},
    "tiny": {"depths": [3, 3, 9, 3], "hidden_sizes": [96, 192, 384, 768]},
    "base": {"depths": [3, 3, 27, 3], "hidden_sizes": [128, 256, 512, 1024]},
    "large": {"depths": [3, 3, 27, 3], "hidden_sizes": [192, 384, 768, 1536]},
    "huge": {"depths": [3, 3, 27, 3], "hidden_sizes": [352, 704, 1408, 2816]},
}
IMAGENET_MEAN = [0.485, 0.456, 0.406]  # pretrained.py:48-49: what _resolve_norm_stats falls back to without an image processor
IMAGENET_STD = [0.229, 0.224, 0.225]
DEFAULT_MODEL_NAME = "facebook/convnextv2-nano-22k-224"
# microsoft/resnet-<N>: layer type, depths, hidden sizes (embedding_size 64 throughout).  The resnet-50 row is ResNetConfig()'s defaults (tests/test_pretrained_resnet_cpu.py
# checks it where transformers is installed); the other rows are the published configs as recalled -- nothing here can reach the hub to check them, a local config.json wins
RESNET_SIZES = {
    "18": {"layer_type": "basic", "depths": [2, 2, 2, 2], "hidden_sizes": [64, 128, 256, 512]},
    "34": {"layer_type": "basic", "depths": [3, 4, 6, 3], "hidden_sizes": [64, 128, 256, 512]},
    "26": {"layer_type": "bottleneck", "depths": [2, 2, 2, 2], "hidden_sizes": [256, 512, 1024, 2048]},
    "50": {"layer_type": "bottleneck", "depths": [3, 4, 6, 3], "hidden_sizes": [256, 512, 1024, 2048]},
    "101": {"layer_type": "bottleneck", "depths": [3, 4, 23, 3], "hidden_sizes": [256, 512, 1024, 2048]},
    "152": {"layer_type": "bottleneck", "depths": [3, 8, 36, 3], "hidden_sizes": [256, 512, 1024, 2048]},
}
RESNET_OPT_IN = ("the ResNet family is opt-in: backbone-config key allow_resnet=True (LoadedAssets.build_model(pretrained_resnet=True), "
                 "Predictor.from_model_paths(..., pretrained_resnet=True))")
BN_EPS = 1e-5  # nn.BatchNorm2d's default, which HuggingFace's ResNetConvLayer keeps
# microsoft/swinv2-<size>-patch4-window<w>-<img>: embed_dim, depths, heads (head dimension 32 throughout).  The tiny row is Swinv2Config()'s defaults
# (tests/test_pretrained_swinv2_cpu.py checks it where transformers is installed); the other rows are the published configs as recalled -- nothing here can reach the hub to
# check them, a local config.json wins.  window_size and image_size come from the id.  pretrained_window_sizes is all zero for a plain id; an id of the form
# window<X>to<Y> (fine-tuned from window X) gets [X, X, X, X // 2] -- the published 12toN configs have [12, 12, 12, 6].  The large row and the <X>to<Y> rule are AS RECALLED
# from HuggingFace's conversion script (convert_swinv2_timm_to_pytorch.py), like the rows above: unconfirmed here, and a local config.json wins over both
SWINV2_SIZES = {
    "tiny": {"embed_dim": 96, "depths": [2, 2, 6, 2], "num_heads": [3, 6, 12, 24]},
    "small": {"embed_dim": 96, "depths": [2, 2, 18, 2], "num_heads": [3, 6, 12, 24]},
    "base": {"embed_dim": 128, "depths": [2, 2, 18, 2], "num_heads": [4, 8, 16, 32]},
    "large": {"embed_dim": 192, "depths": [2, 2, 18, 2], "num_heads": [6, 12, 24, 48]},
}
SWINV2_OPT_IN = ("the Swinv2 family is opt-in: backbone-config key allow_swinv2=True (LoadedAssets.build_model(pretrained_swinv2=True), "
                 "Predictor.from_model_paths(..., pretrained_swinv2=True))")
# effective windows of 9..24 (81..576 tokens: the window16, window12-192, 12to16 and 12to24 checkpoints) run the key-tiled kernel and need a second opt-in on top of that one
SWINV2_WIDE_OPT_IN = ("windows above 8 are opt-in on top of allow_swinv2: backbone-config key allow_swinv2_wide=True (LoadedAssets.build_model(..., swinv2_wide=True), "
                      "Predictor.from_model_paths(..., swinv2_wide=True))")
SWINV2_MAX_WINDOW, SWINV2_MAX_WINDOW_WIDE = 8, 24  # window_attn_kernel's cosine variant holds 64 tokens in one wave; window_attn_v2_wide_kernel tiles the keys of up to 576
SWINV2_HEAD_DIM = 32  # what the cosine attention kernels are built for
SWINV2_MAX_LOGIT = math.log(1.0 / 0.01)  # Swinv2SelfAttention clamps logit_scale here before the exp: scale <= 100


def _refuse(what: str) -> NotImplementedError:
    return NotImplementedError(f"pretrained backbone: {what} is not built on the MI355X path; only the ConvNeXtV2 family in mode='decoder' with all stages is ({THIS_FILE})")


def _resolve_resnet(hf: dict, source: str) -> dict:
    """The ResNet leaf of ``resolve_architecture``: ``hf`` holds config.json's keys (or a row of ``RESNET_SIZES``); what the program cannot run is refused by name."""
    d = RESNET_SIZES["50"]
    arch = {"family": "resnet", "embedding_size": int(hf.get("embedding_size", 64)), "hidden_sizes": [int(v) for v in (hf.get("hidden_sizes") or d["hidden_sizes"])],
            "depths": [int(v) for v in (hf.get("depths") or d["depths"])], "layer_type": str(hf.get("layer_type", "bottleneck")), "num_channels": int(hf.get("num_channels", 3)),
            "patch_size": 4, "drop_path_rate": 0.0, "source": source}
    if hf.get("downsample_in_first_stage", False):
        raise _refuse(f"downsample_in_first_stage=True of {source}")
    if hf.get("downsample_in_bottleneck", False):
        raise _refuse(f"downsample_in_bottleneck=True of {source}")
    if hf.get("hidden_act", "relu") != "relu":
        raise _refuse(f"hidden_act {hf.get('hidden_act')!r} of {source}")
    if arch["layer_type"] not in ("basic", "bottleneck"):
        raise _refuse(f"layer_type {arch['layer_type']!r} of {source}")
    if len(arch["hidden_sizes"]) != 4 or len(arch["depths"]) != 4:
        raise _refuse(f"a ResNet with {len(arch['hidden_sizes'])} stages ({source})")
    return arch


def swinv2_windows(image_size, patch_size: int, window_size: int, n_stages: int = 4) -> List[Tuple[int, int]]:
    """Per stage ``(window, shift of the odd blocks)`` as HuggingFace's ``Swinv2Layer._compute_window_shift`` derives them -- from the CONFIG's ``image_size``, not from the
    frame: stage i has ``input_resolution = image_size // patch_size // 2^i``, ``window = min(resolution, window_size)`` and no shift where the resolution is no larger than
    that window.  (HuggingFace computes both per axis and keeps the height axis' values: ``window_size[0]``, ``shift_size[0]``.)"""
    ih = int(image_size[0] if isinstance(image_size, (list, tuple)) else image_size)
    out = []
    for i in range(n_stages):
        res = ih // int(patch_size) // 2 ** i
        w = min(res, int(window_size))
        out.append((w, 0 if res <= w else int(window_size) // 2))
    return out


def swinv2_coords_table(window: int, pretrained_window: int = 0) -> torch.Tensor:
    """``Swinv2SelfAttention.create_coords_table_and_index``'s table for a square window, ((2w - 1)^2, 2) float32, by the same float32 operations (so the same bits):
    offsets -(w - 1) .. w - 1 over (pretrained_window - 1 if pretrained_window > 0 else w - 1), times 8, then sign(x) log2(|x| + 1) / log2(8).  Row (dy + w - 1)(2w - 1) +
    (dx + w - 1): the index ``relative_position_index`` gives the pair (query - key) = (dy, dx), which is how the attention kernels address their table."""
    r = torch.arange(-(window - 1), window, dtype=torch.int64).float()
    t = torch.stack(torch.meshgrid([r, r], indexing="ij")).permute(1, 2, 0).contiguous().unsqueeze(0)
    if pretrained_window > 0:
        t /= pretrained_window - 1
    elif window > 1:
        t /= window - 1
    t *= 8
    t = torch.sign(t) * torch.log2(torch.abs(t) + 1.0) / math.log2(8)
    return t.view(-1, 2)


def swinv2_bias_table(coords: torch.Tensor, w0: torch.Tensor, b0: torch.Tensor, w2: torch.Tensor) -> torch.Tensor:
    """``16 sigmoid(Linear(512 -> heads, no bias)(relu(Linear(2 -> 512)(coords))))`` in float64, rounded once: (heads, (2w - 1)^2) float32, head-major as the kernel reads it."""
    h = torch.relu(coords.double() @ w0.double().t() + b0.double())
    return (16.0 * torch.sigmoid(h @ w2.double().t())).t().contiguous().float()


def swinv2_logit_scale(logit_scale: torch.Tensor) -> torch.Tensor:
    """``exp(min(logit_scale, log 100))`` per head, float64 rounded once: (heads,) float32."""
    return torch.exp(torch.clamp(logit_scale.double().reshape(-1), max=SWINV2_MAX_LOGIT)).float().contiguous()


def _resolve_swinv2(hf: dict, source: str, allow_wide: bool = False) -> dict:
    """The Swinv2 leaf of ``resolve_architecture``: ``hf`` holds config.json's keys (or a row of ``SWINV2_SIZES`` with the id's window and image size); what the program
    cannot run is refused by name."""
    d = SWINV2_SIZES["tiny"]
    embed = int(hf.get("embed_dim", d["embed_dim"]))
    depths = [int(v) for v in (hf.get("depths") or d["depths"])]
    heads = [int(v) for v in (hf.get("num_heads") or d["num_heads"])]
    img = hf.get("image_size", 224)
    img = [int(v) for v in img] if isinstance(img, (list, tuple)) else [int(img), int(img)]
    ps = hf.get("patch_size", 4)
    ps = int(ps[0] if isinstance(ps, (list, tuple)) else ps)
    ws = int(hf.get("window_size", 7))
    if len(depths) != 4 or len(heads) != 4:
        raise _refuse(f"a Swinv2 with {len(depths)} stages ({source})")
    pws = [int(v) for v in (hf.get("pretrained_window_sizes") or [0, 0, 0, 0])]
    if len(pws) != 4:
        raise _refuse(f"pretrained_window_sizes={pws} of {source} (one per stage)")
    eps = float(hf.get("layer_norm_eps", 1e-5))
    arch = {"family": "swinv2", "embed_dim": embed, "hidden_sizes": [embed * 2 ** i for i in range(4)], "depths": depths, "num_heads": heads, "image_size": img, "patch_size": ps,
            "window_size": ws, "pretrained_window_sizes": pws, "mlp_ratio": float(hf.get("mlp_ratio", 4.0)), "qkv_bias": bool(hf.get("qkv_bias", True)), "layer_norm_eps": eps,
            "num_channels": int(hf.get("num_channels", 3)), "drop_path_rate": float(hf.get("drop_path_rate", 0.1)), "source": source}
    for c, h in zip(arch["hidden_sizes"], heads):
        if h < 1 or c != h * SWINV2_HEAD_DIM:
            raise _refuse(f"a head dimension of {c}/{h} ({source}; the cosine window attention kernel is built for {SWINV2_HEAD_DIM})")
    for i, (w, _s) in enumerate(swinv2_windows(img, ps, ws)):
        if SWINV2_MAX_WINDOW < w <= SWINV2_MAX_WINDOW_WIDE and not allow_wide:
            raise _refuse(f"an effective window of {w} in stage {i + 1} of {source} (window_size {ws}, image_size {img[0]}; {SWINV2_WIDE_OPT_IN}; without it a window above {SWINV2_MAX_WINDOW})")
        if not (2 <= w <= SWINV2_MAX_WINDOW_WIDE):
            raise _refuse(f"an effective window of {w} in stage {i + 1} of {source} (window_size {ws}, image_size {img[0]}; the kernels hold windows of 2..{SWINV2_MAX_WINDOW_WIDE}, "
                          f"at most {SWINV2_MAX_WINDOW_WIDE ** 2} tokens)")
    if hf.get("use_absolute_embeddings", False):
        raise _refuse(f"use_absolute_embeddings=True of {source}")
    if hf.get("hidden_act", "gelu") != "gelu":
        raise _refuse(f"hidden_act {hf.get('hidden_act')!r} of {source}")
    if eps not in (1e-5, 1e-6):
        raise _refuse(f"layer_norm_eps={eps} of {source} (the LayerNorm ops have 1e-5 and 1e-6)")
    if not arch["qkv_bias"]:
        raise _refuse(f"qkv_bias=False of {source} (the padded tokens of a window read their q and v from the biases)")
    if arch["mlp_ratio"] <= 0 or int(arch["mlp_ratio"] * embed) != arch["mlp_ratio"] * embed:
        raise _refuse(f"mlp_ratio={arch['mlp_ratio']} of {source}")
    return arch


def resolve_architecture(model_name: str, run_dir: Optional[str] = None, allow_resnet: bool = False, allow_swinv2: bool = False, allow_swinv2_wide: bool = False) -> dict:
    """``model_name`` -> {"family", "depths", "hidden_sizes", "patch_size", "num_channels", ...} without touching a network.

    (a) a directory holding a ``config.json`` (absolute as given; relative against ``run_dir``, then the working directory), dispatched on its ``model_type``;
    (b) the size word of a ``convnextv2-<size>`` id, or -- with ``allow_resnet`` -- the number of a ``resnet-<N>`` id, or -- with ``allow_swinv2`` -- size, window and image
    size of a ``swinv2-<size>-patch4-window<w>-<img>`` id (effective windows above 8 with ``allow_swinv2_wide`` on top, which alone opens nothing); (c) anything else is
    refused."""
    name = str(model_name)
    cands = [name] if os.path.isabs(name) else ([os.path.join(run_dir, name)] if run_dir else []) + [os.path.join(os.getcwd(), name)]
    for d in cands:
        path = os.path.join(d, "config.json")
        if not os.path.isfile(path):
            continue
        with open(path) as f:
            hf = json.load(f)
        mt = hf.get("model_type")
        if mt == "resnet" and allow_resnet:
            return _resolve_resnet(hf, path)
        if mt == "swinv2" and allow_swinv2:
            return _resolve_swinv2(hf, path, allow_swinv2_wide)
        if mt != "convnextv2":
            raise _refuse(f"model_type {mt!r} of {path}" + (f" ({RESNET_OPT_IN})" if mt == "resnet" else f" ({SWINV2_OPT_IN})" if mt == "swinv2" else ""))
        if hf.get("hidden_act", "gelu") != "gelu":
            raise _refuse(f"hidden_act {hf.get('hidden_act')!r} of {path}")
        eps = float(hf.get("layer_norm_eps", 1e-12))  # (the classifier's pooled norm: no op of the backbone reads it)
        depths = [int(v) for v in (hf.get("depths") or CONVNEXTV2_SIZES["tiny"]["depths"])]
        hidden = [int(v) for v in (hf.get("hidden_sizes") or CONVNEXTV2_SIZES["tiny"]["hidden_sizes"])]
        return {"family": "convnextv2", "depths": depths, "hidden_sizes": hidden, "patch_size": int(hf.get("patch_size", 4)), "num_channels": int(hf.get("num_channels", 3)),
                "layer_norm_eps": eps, "drop_path_rate": float(hf.get("drop_path_rate", 0.0)), "source": path}
    m = re.search(r"convnextv2-([a-z]+)", name.lower())
    if m and m.group(1) in CONVNEXTV2_SIZES:
        a = CONVNEXTV2_SIZES[m.group(1)]
        return {"family": "convnextv2", "depths": list(a["depths"]), "hidden_sizes": list(a["hidden_sizes"]), "patch_size": 4, "num_channels": 3, "layer_norm_eps": 1e-12,
                "drop_path_rate": 0.0, "source": m.group(0)}
    r = re.search(r"resnet-(\d+)", name.lower())
    if r and r.group(1) in RESNET_SIZES and allow_resnet:
        return _resolve_resnet(RESNET_SIZES[r.group(1)], r.group(0))
    # (window12to16-192to256: the fine-tuned window and image size; the window it was pre-trained at normalises the coordinate table)
    s = re.search(r"swinv2-(tiny|small|base|large)-patch4-window(?:(\d+)to)?(\d+)-(?:\d+to)?(\d+)", name.lower())
    if s and allow_swinv2:
        pre = int(s.group(2)) if s.group(2) else 0
        return _resolve_swinv2({**SWINV2_SIZES[s.group(1)], "window_size": int(s.group(3)), "image_size": int(s.group(4)), "patch_size": 4,
                                "pretrained_window_sizes": [pre, pre, pre, pre // 2]}, s.group(0), allow_swinv2_wide)
    hint = f"; {RESNET_OPT_IN}" if r and r.group(1) in RESNET_SIZES else f"; {SWINV2_OPT_IN}" if s else ""
    raise _refuse(f"model_name {name!r} (no local config.json, not a convnextv2-<size> id: ResNet, Swinv2, DINO and the isotropic ViTs are other families{hint})")


def fold_batchnorm(w: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, mean: torch.Tensor, var: torch.Tensor, eps: float = BN_EPS) -> Tuple[torch.Tensor, torch.Tensor]:
    """conv (no bias) -> BatchNorm2d in eval mode as one conv: (W * s[:, None, None, None], beta - mean * s) with s = gamma / sqrt(var + eps), computed in float64."""
    s = gamma.double() / torch.sqrt(var.double() + eps)
    return (w.double() * s.view(-1, 1, 1, 1)).float().contiguous(), (beta.double() - mean.double() * s).float().contiguous()


@dataclass
class PretrainedBackbone:
    """Config-derived description; ``from_config`` mirrors pretrained.py:436-461."""

    source: str = "hf"
    model_name: str = DEFAULT_MODEL_NAME
    in_channels: int = 3
    output_stride: int = 2
    weights: bool = True  # ignored: the checkpoint supplies the weights
    mode: str = "auto"
    out_indices: Optional[List[int]] = None
    freeze: bool = False  # the reference's freeze_encoder(): backbone.enc.* gets no gradient and no optimizer update (TrainingModule)
    drop_path_rate: float = 0.0  # config.json's; the eval forward ignores it, a non-zero value is refused when training is switched on
    revision: Optional[str] = None  # accepted, unused (nothing is downloaded)
    normalize: bool = True
    image_mean: Optional[List[float]] = None
    image_std: Optional[List[float]] = None
    filters_rate: float = 2.0
    convs_per_block: int = 2
    kernel_size: int = 3
    up_interpolate: bool = True
    depths: List[int] = field(default_factory=list)
    channels: List[int] = field(default_factory=list)
    patch_size: int = 4
    ops: List[OpSpec] = field(default_factory=list)
    n_slots: int = 0
    decoder_stride_to_filters: Dict[int, int] = field(default_factory=dict)
    decoder_slot_of_stride: Dict[int, int] = field(default_factory=dict)
    middle_slot: int = -1
    param_shapes: Dict[str, Tuple[int, ...]] = field(default_factory=dict)
    labels: Dict[str, int] = field(default_factory=dict)
    # checkpoint entries that are not parameters.  Unlike Swin's index buffers these are READ from the checkpoint (loaded_buffers): the values a run was
    # trained with override what the config or the ImageNet default would give
    buffers: Dict[str, torch.Tensor] = field(default_factory=dict)
    loaded_buffers: Tuple[str, ...] = ("backbone.image_mean", "backbone.image_std")
    # ResNet family (HuggingFace ResNetBackbone; opt-in through the config key allow_resnet).  BatchNorm never reaches the program: `bn_convs` lists every conv as
    # (conv weight key, BatchNorm prefix) and `folded_params` gives the two tensors its op reads in place of <conv>.weight and <bn>.bias.  The running statistics are
    # loaded_buffers (read from the checkpoint); num_batches_tracked is in every checkpoint, accepted and ignored (ignored_buffers)
    family: str = "convnextv2"
    embedding_size: int = 64
    layer_type: str = "bottleneck"
    bn_convs: List[Tuple[str, str]] = field(default_factory=list)
    ignored_buffers: Tuple[str, ...] = ()
    unit_init_keys: Tuple[str, ...] = ()  # parameters init_xavier_ sets to 1 (BatchNorm weights)
    # Swinv2 family (HuggingFace Swinv2Backbone; opt-in through the config key allow_swinv2).  `swinv2_blocks` lists every block as (name, heads, window, pretrained window):
    # `derived_params` gives the tensors its qkv Linear and its attention op read in place of query.weight / query.bias / continuous_position_bias_mlp.2.weight / logit_scale
    embed_dim: int = 96
    num_heads: List[int] = field(default_factory=list)
    window_size: int = 7
    image_size: List[int] = field(default_factory=lambda: [224, 224])
    pretrained_window_sizes: List[int] = field(default_factory=lambda: [0, 0, 0, 0])
    mlp_ratio: float = 4.0
    layer_norm_eps: float = 1e-5
    swinv2_blocks: List[Tuple[str, int, int, int]] = field(default_factory=list)

    @classmethod
    def from_config(cls, config) -> "PretrainedBackbone":
        source = cfg_get(config, "source", "hf")
        if source != "hf":
            raise ValueError(f"Unsupported pretrained backbone source: {source!r}. Only 'hf' (HuggingFace transformers) is currently supported.")
        mode = cfg_get(config, "mode", "auto")
        if mode not in ("auto", "decoder"):
            raise _refuse(f"mode={mode!r} (the encoder-only pooled bottleneck)")
        name = cfg_get(config, "model_name", None) or DEFAULT_MODEL_NAME
        arch = resolve_architecture(name, cfg_get(config, "_run_dir", None), allow_resnet=bool(cfg_get(config, "allow_resnet", False)),
                                    allow_swinv2=bool(cfg_get(config, "allow_swinv2", False)), allow_swinv2_wide=bool(cfg_get(config, "allow_swinv2_wide", False)))
        oi = cfg_get(config, "out_indices", None)
        if oi is not None and [int(i) for i in oi] != [0, 1, 2, 3, 4]:
            raise _refuse(f"out_indices={list(oi)} (a subset of the stages)")
        in_channels = int(cfg_get(config, "in_channels", 3))
        if in_channels != arch["num_channels"]:
            raise _refuse(f"in_channels={in_channels} for {name}, whose stem takes {arch['num_channels']} channels (gray frames are replicated by Model.forward; keep in_channels at {arch['num_channels']}),")
        mean, std = cfg_get(config, "image_mean", None), cfg_get(config, "image_std", None)
        net = cls(
            source=source, model_name=str(name), in_channels=in_channels, output_stride=int(cfg_get(config, "output_stride", 2)),
            weights=bool(cfg_get(config, "weights", True)), mode=mode, out_indices=None if oi is None else [int(i) for i in oi],
            freeze=bool(cfg_get(config, "freeze", False)), revision=cfg_get(config, "revision", None), normalize=bool(cfg_get(config, "normalize", True)),
            image_mean=None if mean is None else [float(v) for v in mean], image_std=None if std is None else [float(v) for v in std],
            filters_rate=cfg_get(config, "filters_rate", 2.0), convs_per_block=int(cfg_get(config, "convs_per_block", 2)),
            kernel_size=int(cfg_get(config, "kernel_size", 3)), up_interpolate=bool(cfg_get(config, "up_interpolate", True)),
            depths=[int(d) for d in arch["depths"]], channels=[int(c) for c in arch["hidden_sizes"]], patch_size=int(arch["patch_size"]),
            drop_path_rate=float(arch.get("drop_path_rate", 0.0)), family=str(arch.get("family", "convnextv2")), embedding_size=int(arch.get("embedding_size", 64)),
            layer_type=str(arch.get("layer_type", "bottleneck")), embed_dim=int(arch.get("embed_dim", 96)), num_heads=[int(h) for h in arch.get("num_heads", [])],
            window_size=int(arch.get("window_size", 7)), image_size=[int(v) for v in arch.get("image_size", [224, 224])],
            pretrained_window_sizes=[int(v) for v in arch.get("pretrained_window_sizes", [0, 0, 0, 0])], mlp_ratio=float(arch.get("mlp_ratio", 4.0)),
            layer_norm_eps=float(arch.get("layer_norm_eps", 1e-5)),
        )
        net._build()
        return net

    @property
    def max_stride(self) -> int:
        return self.patch_size * 2 ** (len(self.channels) - 1)  # the probed deepest stride (pretrained.py:353-362): 32

    @property
    def max_channels(self) -> int:
        return int(self.channels[-1])  # middle_blocks[-1].filters: the bottleneck (pretrained.py:403-404)

    def encoder_ops(self) -> int:
        """Number of leading ops of the program that belong to the encoder (everything up to the last op with a ``backbone.enc.*`` parameter): the
        frozen prefix of ``ph_model_backward`` (handle option ``bwd_frozen_ops``) under ``freeze``."""
        return 1 + max(i for i, o in enumerate(self.ops) if (o.weight or "").startswith("backbone.enc."))

    def check_trainable(self) -> None:
        """What the opt-in to training refuses by name."""
        if self.family == "resnet":
            raise _refuse("training a ResNet backbone (BatchNorm with batch statistics is another op; the program runs the eval fold only)")
        if self.family == "swinv2":
            raise _refuse("training a Swinv2 backbone (the cosine window attention, the residual-after-norm LayerNorm and the norm-less patch merge have no backward step; "
                          "the program is the eval forward only)")
        if self.drop_path_rate != 0.0:
            raise _refuse(f"training with drop_path_rate={self.drop_path_rate} (stochastic depth of the ConvNeXtV2 blocks; the published configs have 0.0)")

    def norm_stats(self) -> Tuple[List[float], List[float]]:
        """pretrained.py:270-297 without the image processor (a network read): explicit values, identity when disabled, else ImageNet."""
        if self.image_mean is not None and self.image_std is not None:
            return list(self.image_mean), list(self.image_std)
        if not self.normalize:
            return [0.0] * self.in_channels, [1.0] * self.in_channels
        return list(IMAGENET_MEAN), list(IMAGENET_STD)

    # -- program construction ---------------------------------------------------------
    def _new_slot(self) -> int:
        self.n_slots += 1
        return self.n_slots - 1

    def _emit(self, op: OpSpec) -> int:
        op.flags |= L.FLAG_NO_TRAIN if op.kind in (L.OP_GRN, L.OP_PATCH_STEM) else 0
        self.ops.append(op)
        return op.dst

    def _conv3(self, name: str, src0: int, cin0: int, cout: int, src1: int = -1, cin1: int = 0) -> int:
        dst = self._new_slot()
        self.param_shapes[name + ".weight"] = (cout, cin0 + cin1, 3, 3)
        self.param_shapes[name + ".bias"] = (cout,)
        self.ops.append(OpSpec(L.OP_CONV, src0, src1, dst, cin0, cin1, cout, 3, L.FLAG_RELU, name + ".weight", name + ".bias", label=name))
        self.labels[name] = dst
        return dst

    def _layernorm(self, name: str, src: int, c: int) -> int:
        self.param_shapes[name + ".weight"] = (c,)
        self.param_shapes[name + ".bias"] = (c,)
        return self._emit(OpSpec(L.OP_LAYERNORM, src, -1, self._new_slot(), c, 0, c, 1, 0, name + ".weight", name + ".bias", label=name))

    def _v2_block(self, name: str, x: int, c: int) -> int:
        p = self.param_shapes
        p[name + ".dwconv.weight"] = (c, 1, 7, 7)
        p[name + ".dwconv.bias"] = (c,)
        y = self._emit(OpSpec(L.OP_DWCONV, x, -1, self._new_slot(), c, 0, c, 7, 0, name + ".dwconv.weight", name + ".dwconv.bias", label=name + ".dwconv"))
        y = self._layernorm(name + ".layernorm", y, c)
        p[name + ".pwconv1.weight"] = (4 * c, c)
        p[name + ".pwconv1.bias"] = (4 * c,)
        y = self._emit(OpSpec(L.OP_LINEAR, y, -1, self._new_slot(), c, 0, 4 * c, 1, 0, name + ".pwconv1.weight", name + ".pwconv1.bias", label=name + ".pwconv1"))
        y = self._emit(OpSpec(L.OP_GELU, y, -1, self._new_slot(), 4 * c, 0, 4 * c, 1, 0, label=name + ".act"))
        p[name + ".grn.weight"] = (1, 1, 1, 4 * c)
        p[name + ".grn.bias"] = (1, 1, 1, 4 * c)
        y = self._emit(OpSpec(L.OP_GRN, y, -1, self._new_slot(), 4 * c, 0, 4 * c, 1, 0, name + ".grn.weight", name + ".grn.bias", label=name + ".grn"))
        self.labels[name + ".grn"] = y
        p[name + ".pwconv2.weight"] = (c, 4 * c)
        p[name + ".pwconv2.bias"] = (c,)
        # no layer scale; drop path is the identity in eval and at drop_path_rate 0 (the only rate that trains here): the residual add is the GEMM's PH_FLAG_RESIDUAL epilogue
        y = self._emit(OpSpec(L.OP_LINEAR, y, x, self._new_slot(), 4 * c, 0, c, 1, L.FLAG_RESIDUAL, name + ".pwconv2.weight", name + ".pwconv2.bias", label=name))
        self.labels[name] = y
        return y

    def _build(self) -> None:
        if self.kernel_size != 3:
            raise ValueError("only kernel_size=3 is supported by the MFMA convolution kernels")
        if len(self.channels) != 4 or len(self.depths) != 4:
            raise _refuse(f"a ConvNeXtV2 with {len(self.channels)} stages")
        if not (2 <= self.patch_size <= 8):
            raise ValueError("patch_size must be in 2..8")
        if self.in_channels < 1 or self.in_channels > 4:
            raise ValueError("in_channels must be in 1..4")
        mean, std = self.norm_stats()
        self.buffers = {"backbone.image_mean": torch.tensor(mean, dtype=torch.float32).view(1, -1, 1, 1),
                        "backbone.image_std": torch.tensor(std, dtype=torch.float32).view(1, -1, 1, 1)}
        if self.family == "resnet":
            self._build_resnet_encoder()
        elif self.family == "swinv2":
            self._build_swinv2_encoder()
        else:
            self._build_encoder()

    # -- ResNet (HuggingFace ResNetBackbone): embedder (7x7 s2 conv + BN + ReLU, 3x3 s2 max pool), four stages of basic / bottleneck layers, RAW stage outputs as the pyramid
    def _bn_conv(self, name: str, cout: int, cin: int, k: int) -> Tuple[str, str]:
        """Register ``<name>.convolution`` (bias-less) + ``<name>.normalization``; -> the keys the conv's op reads as weight and bias (both folded at handle creation)."""
        cw, bn = name + ".convolution.weight", name + ".normalization"
        self.param_shapes[cw] = (cout, cin, k, k)
        self.param_shapes[bn + ".weight"] = (cout,)
        self.param_shapes[bn + ".bias"] = (cout,)
        self.buffers[bn + ".running_mean"] = torch.zeros(cout)
        self.buffers[bn + ".running_var"] = torch.ones(cout)
        self.buffers[bn + ".num_batches_tracked"] = torch.zeros((), dtype=torch.int64)
        self.bn_convs.append((cw, bn))
        return cw, bn + ".bias"

    def _rn_conv(self, name: str, x: int, cin: int, cout: int, k: int, stride: int, relu: bool, residual: int = -1) -> int:
        """One ResNetConvLayer / ResNetShortCut as the op that runs it: 1x1 s1 -> Linear (row GEMM), 3x3 s1 -> PH_OP_CONV, anything at stride 2 -> PH_OP_CONV_S2."""
        w, b = self._bn_conv(name, cout, cin, k)
        act = L.FLAG_RELU if relu else 0
        dst = self._new_slot()
        if stride == 2:
            op = OpSpec(L.OP_CONV_S2, x, -1, dst, cin, 0, cout, k, act | L.FLAG_NO_TRAIN, w, b, label=name)
        elif k == 1:
            op = OpSpec(L.OP_LINEAR, x, residual, dst, cin, 0, cout, 1, act | (L.FLAG_RESIDUAL if residual >= 0 else 0), w, b, label=name)
        else:
            op = OpSpec(L.OP_CONV, x, -1, dst, cin, 0, cout, 3, act, w, b, label=name)
        self.ops.append(op)
        self.labels[name] = dst
        return dst

    def _rn_layer(self, name: str, x: int, cin: int, cout: int, stride: int) -> int:
        res = self._rn_conv(name + ".shortcut", x, cin, cout, 1, stride, relu=False) if (cin != cout or stride != 1) else x
        if self.layer_type == "bottleneck":
            r = cout // 4  # (HuggingFace's `out_channels // reduction`: 18 -> 4)
            y = self._rn_conv(name + ".layer.0", x, cin, r, 1, 1, relu=True)
            y = self._rn_conv(name + ".layer.1", y, r, r, 3, stride, relu=True)
            y = self._rn_conv(name + ".layer.2", y, r, cout, 1, 1, relu=True, residual=res)  # relu(conv + bias + shortcut): the row GEMM's residual-then-ReLU epilogue
        else:
            y = self._rn_conv(name + ".layer.0", x, cin, cout, 3, stride, relu=True)
            y = self._rn_conv(name + ".layer.1", y, cout, cout, 3, 1, relu=False)
            dst = self._new_slot()
            self.ops.append(OpSpec(L.OP_ADD_RELU, y, res, dst, cout, 0, cout, 1, L.FLAG_NO_TRAIN, label=name))
            y = dst
        self.labels[name] = y
        return y

    def _build_resnet_encoder(self) -> None:
        enc = "backbone.enc"
        name = f"{enc}.embedder.embedder"
        w, b = self._bn_conv(name, self.embedding_size, self.in_channels, 7)
        full, pooled = self._new_slot(), self._new_slot()
        self.ops.append(OpSpec(L.OP_RESNET_STEM, -1, -1, full, self.in_channels, 0, self.embedding_size, 7, L.FLAG_RELU | L.FLAG_NO_TRAIN, w, b, label=name, dst2=pooled))
        self.labels[name] = full
        self.labels[f"{enc}.embedder"] = pooled  # feature map "stem": stride 4, like stage1, and dropped by the reference's stride dedupe
        x, cin = pooled, self.embedding_size
        feats: List[Tuple[int, int]] = []
        for si, (depth, c) in enumerate(zip(self.depths, self.channels)):
            for j in range(depth):
                x = self._rn_layer(f"{enc}.encoder.stages.{si}.layers.{j}", x, cin, c, 2 if (si > 0 and j == 0) else 1)
                cin = c
            self.labels[f"{enc}.stage{si + 1}"] = x
            feats.append((x, c))  # the RAW stage output: no output norms, unlike ConvNeXtV2
        bn_keys = [k for k in self.buffers if ".normalization." in k]
        self.loaded_buffers = tuple(self.loaded_buffers) + tuple(k for k in bn_keys if not k.endswith("num_batches_tracked"))
        self.ignored_buffers = tuple(k for k in bn_keys if k.endswith("num_batches_tracked"))
        self.unit_init_keys = tuple(bn + ".weight" for _w, bn in self.bn_convs)
        self._build_decoder(feats)

    def folded_params(self, state: Dict[str, torch.Tensor], buffers: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
        """BatchNorm (eval) folded into the conv in front of it, per output channel: W' = W * g / sqrt(var + eps) under the conv's weight key and
        b' = beta - mean * g / sqrt(var + eps) under the BatchNorm's bias key -- the two keys the conv's op reads.  float64 on the host, rounded once to float32."""
        out: Dict[str, torch.Tensor] = {}
        for cw, bn in self.bn_convs:
            out[cw], out[bn + ".bias"] = fold_batchnorm(state[cw], state[bn + ".weight"], state[bn + ".bias"], buffers[bn + ".running_mean"], buffers[bn + ".running_var"])
        return out

    # -- Swinv2 (HuggingFace Swinv2Backbone): padding-0 patch stem + LayerNorm, four stages of cosine-attention blocks that norm AFTER each branch, patch merging between
    # them (gather -> bias-less reduction -> LayerNorm), RAW stage outputs (before the downsampling) as the pyramid
    def _sv2_linear(self, name: str, src: int, cin: int, cout: int, weight: Optional[str] = None, bias: Optional[str] = None) -> int:
        return self._emit(OpSpec(L.OP_LINEAR, src, -1, self._new_slot(), cin, 0, cout, 1, 0, weight or name + ".weight", bias, label=name))

    def _sv2_norm(self, name: str, src: int, c: int, eps: float, residual: int = -1) -> int:
        flags = (L.FLAG_LN_EPS_1EM5 if eps == 1e-5 else 0) | ((L.FLAG_RESIDUAL | L.FLAG_NO_TRAIN) if residual >= 0 else 0)
        return self._emit(OpSpec(L.OP_LAYERNORM, src, residual, self._new_slot(), c, 0, c, 1, flags, name + ".weight", name + ".bias", label=name))

    def _swinv2_block(self, name: str, x: int, c: int, heads: int, window: int, shift: int, pretrained_window: int) -> int:
        p = self.param_shapes
        a = name + ".attention.self"
        hid = int(self.mlp_ratio * c)
        # registered in the order of Swinv2Layer.__init__ (parameter arena = state_dict order), whatever the order the ops read them in
        p[a + ".logit_scale"] = (heads, 1, 1)
        p[a + ".continuous_position_bias_mlp.0.weight"] = (512, 2)
        p[a + ".continuous_position_bias_mlp.0.bias"] = (512,)
        p[a + ".continuous_position_bias_mlp.2.weight"] = (heads, 512)
        p[a + ".query.weight"] = (c, c)
        p[a + ".query.bias"] = (c,)
        p[a + ".key.weight"] = (c, c)
        p[a + ".value.weight"] = (c, c)
        p[a + ".value.bias"] = (c,)
        for n, (co, ci) in ((name + ".attention.output.dense", (c, c)), (name + ".layernorm_before", (c, 0)), (name + ".intermediate.dense", (hid, c)),
                            (name + ".output.dense", (c, hid)), (name + ".layernorm_after", (c, 0))):
            p[n + ".weight"] = (co, ci) if ci else (co,)
            p[n + ".bias"] = (co,)
        self.swinv2_blocks.append((name, heads, window, pretrained_window))
        # the qkv Linear and the attention op read DERIVED tensors under four of these keys (derived_params): query.weight -> (3C, C) query | key | value,
        # query.bias -> (3C) query.bias | 0 | value.bias, continuous_position_bias_mlp.2.weight -> the (heads, (2w - 1)^2) bias table, logit_scale -> the (heads) scales
        qkv = self._sv2_linear(a + ".qkv", x, c, 3 * c, weight=a + ".query.weight", bias=a + ".query.bias")
        y = self._emit(OpSpec(L.OP_WINDOW_ATTN_V2, qkv, -1, self._new_slot(), 3 * c, heads, c, window, L.FLAG_NO_TRAIN, a + ".continuous_position_bias_mlp.2.weight",
                              a + ".query.bias", label=a, cmid=shift, weight2=a + ".logit_scale"))
        self.labels[a] = y
        y = self._sv2_linear(name + ".attention.output.dense", y, c, c, bias=name + ".attention.output.dense.bias")
        self.labels[name + ".attention"] = y
        x1 = self._sv2_norm(name + ".layernorm_before", y, c, self.layer_norm_eps, residual=x)  # x + LayerNorm(attention(x)): drop path is the identity in eval
        self.labels[name + ".layernorm_before"] = x1
        y = self._sv2_linear(name + ".intermediate.dense", x1, c, hid, bias=name + ".intermediate.dense.bias")
        y = self._emit(OpSpec(L.OP_GELU, y, -1, self._new_slot(), hid, 0, hid, 1, 0, label=name + ".intermediate"))  # (Model folds it into the GEMM's epilogue)
        self.labels[name + ".intermediate"] = y
        y = self._sv2_linear(name + ".output.dense", y, hid, c, bias=name + ".output.dense.bias")
        self.labels[name + ".output"] = y
        x2 = self._sv2_norm(name + ".layernorm_after", y, c, self.layer_norm_eps, residual=x1)
        self.labels[name] = x2
        return x2

    def _build_swinv2_encoder(self) -> None:
        ch = self.channels
        enc = "backbone.enc"
        pe = f"{enc}.embeddings.patch_embeddings.projection"
        self.param_shapes[pe + ".weight"] = (ch[0], self.in_channels, self.patch_size, self.patch_size)
        self.param_shapes[pe + ".bias"] = (ch[0],)
        x = self._emit(OpSpec(L.OP_PATCH_STEM, -1, -1, self._new_slot(), self.in_channels, 0, ch[0], self.patch_size, L.FLAG_PAD0_NORM, pe + ".weight", pe + ".bias",
                              label=pe, cmid=self.patch_size))
        self.labels[pe] = x
        self.param_shapes[f"{enc}.embeddings.norm.weight"] = (ch[0],)
        self.param_shapes[f"{enc}.embeddings.norm.bias"] = (ch[0],)
        x = self._sv2_norm(f"{enc}.embeddings.norm", x, ch[0], 1e-5)  # nn.LayerNorm(embed_dim): the module default, whatever layer_norm_eps says
        self.labels[f"{enc}.embeddings"] = x  # feature map "stem": stride 4, like stage1, and dropped by the reference's stride dedupe
        windows = swinv2_windows(self.image_size, self.patch_size, self.window_size)
        feats: List[Tuple[int, int]] = []
        for si, (depth, c) in enumerate(zip(self.depths, ch)):
            w, shift = windows[si]
            for j in range(depth):
                x = self._swinv2_block(f"{enc}.encoder.layers.{si}.blocks.{j}", x, c, self.num_heads[si], w, 0 if j % 2 == 0 else shift, self.pretrained_window_sizes[si])
            self.labels[f"{enc}.stage{si + 1}"] = x
            feats.append((x, c))  # the RAW stage output, before the downsampling: no output norms
            if si + 1 < len(ch):
                name = f"{enc}.encoder.layers.{si}.downsample"
                self.param_shapes[name + ".reduction.weight"] = (2 * c, 4 * c)
                self.param_shapes[name + ".norm.weight"] = (2 * c,)
                self.param_shapes[name + ".norm.bias"] = (2 * c,)
                # the phase order is HuggingFace's = torchvision's: (even, even), (odd, even), (even, odd), (odd, odd) in (row, column); no norm in front of the reduction
                y = self._emit(OpSpec(L.OP_PATCH_MERGE, x, -1, self._new_slot(), c, 0, 4 * c, 2, L.FLAG_NO_NORM | L.FLAG_NO_TRAIN, label=name + ".gather"))
                y = self._sv2_linear(name + ".reduction", y, 4 * c, 2 * c)
                self.labels[name + ".reduction"] = y
                x = self._sv2_norm(name + ".norm", y, 2 * c, 1e-5)  # norm_layer(2 * dim) = nn.LayerNorm's default eps
                self.labels[name] = x
        self._build_decoder(feats)

    def derived_params(self, state: Dict[str, torch.Tensor], buffers: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
        """The tensors a Swinv2 block's qkv Linear and attention op read in place of four of its parameters, computed in float64 at handle creation and rounded once:
        ``query.weight`` -> (3C, C) query | key | value; ``query.bias`` -> (3C) query.bias | zeros | value.bias (``key`` has no bias; also the q, k, v of a padded token);
        ``continuous_position_bias_mlp.2.weight`` -> ``16 sigmoid(MLP(coords))`` as (heads, (2w - 1)^2); ``logit_scale`` -> ``exp(min(logit_scale, log 100))`` as (heads,).
        The state dict keeps the reference's tensors; ``load_state_dict`` releases the handle, so a derived form never outlives what it was made from."""
        out: Dict[str, torch.Tensor] = {}
        for name, _heads, window, pretrained_window in self.swinv2_blocks:
            a = name + ".attention.self"
            out[a + ".query.weight"] = torch.cat([state[a + ".query.weight"], state[a + ".key.weight"], state[a + ".value.weight"]], dim=0).float().contiguous()
            qb, vb = state[a + ".query.bias"], state[a + ".value.bias"]
            out[a + ".query.bias"] = torch.cat([qb, torch.zeros_like(qb), vb]).float().contiguous()
            m = a + ".continuous_position_bias_mlp"
            out[m + ".2.weight"] = swinv2_bias_table(swinv2_coords_table(window, pretrained_window), state[m + ".0.weight"], state[m + ".0.bias"], state[m + ".2.weight"])
            out[a + ".logit_scale"] = swinv2_logit_scale(state[a + ".logit_scale"])
        return out

    def _build_encoder(self) -> None:
        ch = self.channels
        enc = "backbone.enc"
        hn = f"{enc}.hidden_states_norms"
        pe = f"{enc}.embeddings.patch_embeddings"
        # embeddings: (x - mean) / std -> Conv2d(patch, stride patch, padding 0) -> LayerNorm (channels first)
        self.param_shapes[pe + ".weight"] = (ch[0], self.in_channels, self.patch_size, self.patch_size)
        self.param_shapes[pe + ".bias"] = (ch[0],)
        x = self._emit(OpSpec(L.OP_PATCH_STEM, -1, -1, self._new_slot(), self.in_channels, 0, ch[0], self.patch_size, L.FLAG_PAD0_NORM, pe + ".weight", pe + ".bias",
                              label=pe, cmid=self.patch_size))
        x = self._layernorm(f"{enc}.embeddings.layernorm", x, ch[0])
        self.labels[f"{enc}.embeddings"] = x
        feats: List[Tuple[int, int]] = []  # (normed map slot, channels), finest first
        for si, (depth, c) in enumerate(zip(self.depths, ch)):
            st = f"{enc}.encoder.stages.{si}"
            if si > 0:
                x = self._layernorm(f"{st}.downsampling_layer.0", x, ch[si - 1])
                name = f"{st}.downsampling_layer.1"
                self.param_shapes[name + ".weight"] = (c, ch[si - 1], 2, 2)
                self.param_shapes[name + ".bias"] = (c,)
                x = self._emit(OpSpec(L.OP_PATCH_CONV, x, -1, self._new_slot(), ch[si - 1], 0, c, 2, 0, name + ".weight", name + ".bias", label=name))
            for j in range(depth):
                x = self._v2_block(f"{st}.layers.{j}", x, c)
            # the map that leaves the encoder is normed; the stream into the next stage is not
            f = self._layernorm(f"{hn}.stage{si + 1}", x, c)
            self.labels[f"{hn}.stage{si + 1}"] = f
            feats.append((f, c))
        # the stem map shares stride 4 with stage1 and is dropped by the stride dedupe (pretrained.py:315-334): its norm is in every checkpoint, loads, and no op reads it
        self.param_shapes[f"{hn}.stem.weight"] = (ch[0],)
        self.param_shapes[f"{hn}.stem.bias"] = (ch[0],)
        self._build_decoder(feats)

    def _build_decoder(self, feats: List[Tuple[int, int]]) -> None:
        """pretrained.py:336-404 + encoder_decoder.py:634-703: no additional pool, no middle blocks; Decoder(stem_blocks=1, down_blocks=n_skips - 1,
        filters=channels[0], encoder_channels=channels[:-1][::-1], prefix="pretrained_dec"); blocks past the skips take the no-concat path with ONE refine conv."""
        ch = self.channels
        cur, cur_c = feats[-1]
        self.middle_slot = cur
        stride = self.max_stride
        up_blocks = int(math.log2(stride / self.output_stride))
        if up_blocks < 1:
            raise ValueError(f"output_stride={self.output_stride} is >= the backbone's deepest stride {stride}; nothing to decode. Lower output_stride.")
        skips = feats[:-1][::-1]  # deepest first
        n_skips = len(skips)
        self.decoder_stride_to_filters = {stride: cur_c}
        for b in range(up_blocks):
            fout = int(ch[0] * (self.filters_rate ** max(0, n_skips - 1 - b)))
            nxt = stride // 2
            name = f"backbone.dec.decoder_stack.{b}.blocks.pretrained_dec{b}_s{stride}_to_s{nxt}"
            concat = b < n_skips
            dst = self._new_slot()
            if self.up_interpolate:
                self.ops.append(OpSpec(L.OP_UPSAMPLE, cur, -1, dst, cur_c, label=name + "_interp_bilinear"))
                up_c = cur_c
            else:
                tn = name + "_trans_conv"
                self.param_shapes[tn + ".weight"] = (cur_c, fout, 3, 3)
                self.param_shapes[tn + ".bias"] = (fout,)
                self.ops.append(OpSpec(L.OP_CONVT, cur, -1, dst, cur_c, 0, fout, 3, L.FLAG_RELU, tn + ".weight", tn + ".bias", label=tn))
                self.labels[tn] = dst
                up_c = fout
            cur, cur_c = dst, up_c
            for i in range(self.convs_per_block if concat else 1):
                cn = name + f"_refine_conv{i}"
                if i == 0 and concat:
                    sk, sk_c = skips[b]
                    cur = self._conv3(cn, sk, sk_c, fout, src1=cur, cin1=cur_c)  # concat (skip, x)
                else:
                    if i == 0 and cur_c != fout:  # (the reference builds this conv with fout inputs: encoder_decoder.py:476-478)
                        raise ValueError(f"decoder block {b} has no skip and {cur_c} input channels for a conv built with {fout}")
                    cur = self._conv3(cn, cur, cur_c, fout)
                cur_c = fout
            self.decoder_stride_to_filters[nxt] = fout
            self.decoder_slot_of_stride[nxt] = cur
            stride = nxt
