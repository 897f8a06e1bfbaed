"""Training targets rendered on the GPU.

``generate_multiconfmaps`` / ``generate_pafs`` keep the reference's call shapes
(``sleap_nn/data/confidence_maps.py:46-94``, ``sleap_nn/data/edge_maps.py:250-323``) but take a whole
batch ``(B, I, N, 2)`` and run one kernel instead of a Python loop over instances per sample.

The targets of the other trainable model types follow the same rule: ``generate_confmaps`` (single-instance and
centred-instance maps), ``generate_centroids``, ``make_class_vectors``, ``generate_class_maps`` and ``filter_oob_points`` keep
the reference's names, argument names and defaults (``data/confidence_maps.py:8-43``, ``data/instance_centroids.py:65-98``,
``data/identity.py:10-137``, ``data/providers.py:38-69``) and take whole batches.  They dispatch on the tensor's device: a
tensor on the GPU takes the HIP kernels (``ph_render_confmaps``, ``ph_instance_centroids``, ``ph_render_class_maps``), a CPU
tensor a torch implementation of the same contract, which is what the CPU tests pin against the reference's recorded results.
``TargetGenerator`` turns a batch's points into the dict of head targets ``TrainingModule.training_step`` takes, for every
model type that can be trained here.

Not here: cutting the training crops of the top-down model types.  The reference cuts them with a Skia resample
(``data/instance_cropping.py``), whose results could be neither recorded nor pinned without Skia; the centred-instance
targets therefore take points that are already in crop coordinates.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Dict, Optional, Sequence, Tuple

import torch

from sleap_nn_amd import _lib as L


def _grid(size: int, stride: int) -> int:
    return (size + stride - 1) // stride


def generate_multiconfmaps(instances: torch.Tensor, img_hw: Tuple[int, int], sigma: float = 1.5, output_stride: int = 2) -> torch.Tensor:
    """``instances``: (B, I, N, 2) (centroids: (B, I, 2)) on the GPU, NaN = missing -> (B, N, h, w)."""
    L.require_cuda(instances, "instances")
    pts = instances.unsqueeze(-2) if instances.dim() == 3 else instances
    pts = pts.to(torch.float32).contiguous()
    B, I, N, _ = pts.shape
    h, w = _grid(img_hw[0], output_stride), _grid(img_hw[1], output_stride)
    out = torch.empty((B, N, h, w), dtype=torch.float32, device=pts.device)
    with torch.cuda.device(pts.device):
        L.check(L.lib().ph_render_confmaps(C.c_void_p(pts.data_ptr()), B, I, N, int(img_hw[0]), int(img_hw[1]), int(output_stride), float(sigma),
                                           C.c_void_p(out.data_ptr()), L.current_stream_ptr()))
    return out


def generate_pafs(instances: torch.Tensor, img_hw: Tuple[int, int], sigma: float = 1.5, output_stride: int = 2, edge_inds: Sequence[Tuple[int, int]] = ()) -> torch.Tensor:
    """``instances``: (B, I, N, 2) on the GPU -> (B, 2E, h, w) (the reference's ``flatten_channels=True`` layout)."""
    L.require_cuda(instances, "instances")
    pts = instances.to(torch.float32).contiguous()
    B, I, N, _ = pts.shape
    e = torch.tensor([list(x) for x in edge_inds], dtype=torch.int32, device=pts.device).reshape(-1, 2).contiguous()
    E = int(e.shape[0])
    h, w = _grid(img_hw[0], output_stride), _grid(img_hw[1], output_stride)
    out = torch.empty((B, 2 * E, h, w), dtype=torch.float32, device=pts.device)
    with torch.cuda.device(pts.device):
        L.check(L.lib().ph_render_pafs(C.c_void_p(pts.data_ptr()), C.c_void_p(e.data_ptr()), B, I, N, E, int(img_hw[0]), int(img_hw[1]), int(output_stride), float(sigma),
                                       C.c_void_p(out.data_ptr()), L.current_stream_ptr()))
    return out


# ---- targets of the identity and top-down model types -------------------------------------------------------------------------------


def _grid_vectors(img_hw, stride: int, device):
    xv = torch.arange(0, int(img_hw[1]), step=int(stride), dtype=torch.float32, device=device)
    yv = torch.arange(0, int(img_hw[0]), step=int(stride), dtype=torch.float32, device=device)
    return xv, yv


def _gaussians(pts: torch.Tensor, img_hw, sigma: float, stride: int) -> torch.Tensor:
    """torch: ``pts`` (..., 2) -> (..., h, w), the unit Gaussian of width ``sigma * stride`` around each point, 0 for a NaN point."""
    xv, yv = _grid_vectors(img_hw, stride, pts.device)
    x, y = pts[..., 0, None, None], pts[..., 1, None, None]
    g = torch.exp(-((xv.view(1, -1) - x) ** 2 + (yv.view(-1, 1) - y) ** 2) / (2 * (sigma * stride) ** 2))
    return torch.nan_to_num(g)


def generate_confmaps(instance: torch.Tensor, img_hw: Tuple[int, int], sigma: float = 1.5, output_stride: int = 2) -> torch.Tensor:
    """``instance``: (B, N, 2), or (B, I, N, 2) flattened to (B, I * N, 2) as the reference's ``view`` does -> (B, N, h, w) / (B, I * N, h, w):
    one Gaussian per point, zeros for a NaN point."""
    if instance.dim() != 3:
        instance = instance.reshape(instance.shape[0], -1, 2)
    pts = instance.to(torch.float32)
    if not pts.is_cuda or pts.shape[0] == 0:  # (an empty batch launches nothing: the torch form returns the empty result on either device)
        return _gaussians(pts, img_hw, sigma, output_stride)
    return generate_multiconfmaps(pts.unsqueeze(1), img_hw, sigma=sigma, output_stride=output_stride)  # one "instance": the maximum is over itself


def generate_centroids(points: torch.Tensor, anchor_ind: Optional[int] = None) -> torch.Tensor:
    """``points``: (..., N, 2) -> (..., 2): the anchor node where it has both coordinates, else the NaN-ignoring mean of the
    instance's nodes (counted per axis), NaN for an instance without any coordinate."""
    N = int(points.shape[-2])
    if anchor_ind is not None:
        if not -N <= anchor_ind < N:
            raise IndexError(f"anchor_ind {anchor_ind} is out of range for {N} nodes")
        anchor_ind = int(anchor_ind) % N
    pts = points.to(torch.float32).reshape(-1, N, 2).contiguous()
    if pts.is_cuda:
        out = torch.empty((pts.shape[0], 2), dtype=torch.float32, device=pts.device)
        with torch.cuda.device(pts.device):
            L.check(L.lib().ph_instance_centroids(C.c_void_p(pts.data_ptr()), int(pts.shape[0]), N, -1 if anchor_ind is None else anchor_ind,
                                                  C.c_void_p(out.data_ptr()), L.current_stream_ptr()))
    else:
        present = ~torch.isnan(pts)
        mean = torch.where(present, pts, torch.zeros_like(pts)).sum(dim=-2) / present.sum(dim=-2).clamp(min=1).to(pts.dtype)
        out = torch.where(present.any(dim=-1).any(dim=-1, keepdim=True), mean, torch.full_like(mean, float("nan")))
        if anchor_ind is not None:
            anchor = pts[:, anchor_ind]
            out = torch.where(torch.isnan(anchor).any(dim=-1, keepdim=True), out, anchor)
    return out.reshape(points.shape[:-2] + (2,))


def make_class_vectors(class_inds: torch.Tensor, n_classes: int) -> torch.Tensor:
    """``class_inds`` (...,) integer, -1 = no class -> (..., n_classes) int32 one-hot rows, all zero for -1."""
    valid = class_inds >= 0
    rows = torch.nn.functional.one_hot(torch.where(valid, class_inds, torch.zeros_like(class_inds)).long(), num_classes=int(n_classes))
    return (rows * valid.unsqueeze(-1)).to(torch.int32)


def class_map_weights(class_inds: torch.Tensor, num_tracks: int) -> torch.Tensor:
    """The (B, C, I) matrix ``generate_class_maps`` weighs the instance masks with.  The reference RESHAPES each frame's (I, C) one-hot
    class vectors to (C, I) (``data/identity.py:66-69``); that is not a transpose, so for I != C the weight of (class c, instance i)
    is element ``c * I + i`` of the flattened (I, C) rows, not ``onehot[i][c]``.  Kept as the reference has it."""
    B, I = class_inds.shape
    return make_class_vectors(class_inds, num_tracks).to(torch.float32).reshape(B, int(num_tracks), I)


def _class_maps_torch(pts: torch.Tensor, wts: torch.Tensor, img_hw, threshold: float, sigma: float, stride: int) -> torch.Tensor:
    """The class maps in torch ops, on the tensors' device: ``pts`` (B, I, N, 2), ``wts`` (B, C, I) -> (B, C, h, w).  Materialises (B, I, N, h, w)."""
    B, I = pts.shape[:2]
    if I == 0:
        return torch.zeros((B, wts.shape[1], _grid(img_hw[0], stride), _grid(img_hw[1], stride)), dtype=torch.float32, device=pts.device)
    m = _gaussians(pts, img_hw, sigma, stride).amax(dim=2)  # (B, I, h, w)
    mask = torch.where(m > threshold, m / m.sum(dim=1, keepdim=True), torch.zeros_like(m))
    return (mask.unsqueeze(1) * wts[:, :, :, None, None]).amax(dim=2)


def generate_class_maps(instances: torch.Tensor, img_hw: Tuple[int, int], class_inds: torch.Tensor, num_tracks: int, class_map_threshold: float = 0.2,
                        sigma: float = 1.5, output_stride: int = 2, is_centroids: bool = False) -> torch.Tensor:
    """``instances``: (B, I, N, 2), or (B, I, 2) with ``is_centroids``; ``class_inds``: (B, I), -1 = no class -> (B, num_tracks, h, w).
    Instances beyond a frame's count are all-NaN rows with class -1.  Per grid point: each instance's map (maximum of its nodes' Gaussians),
    normalised by the sum over the instances where it exceeds ``class_map_threshold`` and zero elsewhere, then per class the maximum of
    weight * mask over the instances."""
    pts = (instances.unsqueeze(-2) if is_centroids else instances).to(torch.float32).contiguous()
    if pts.dim() != 4 or pts.shape[-1] != 2:
        raise ValueError(f"instances must be (B, I, N, 2), or (B, I, 2) with is_centroids; got {tuple(instances.shape)}")
    B, I, N, _ = pts.shape
    if tuple(class_inds.shape) != (B, I):
        raise ValueError(f"class_inds must be (B, I) = {(B, I)}, got {tuple(class_inds.shape)}")
    if class_map_threshold < 0:
        raise ValueError(f"class_map_threshold must be >= 0, got {class_map_threshold}")
    Cn = int(num_tracks)
    wts = class_map_weights(class_inds.to(pts.device), Cn).contiguous()
    h, w = _grid(img_hw[0], output_stride), _grid(img_hw[1], output_stride)
    if not pts.is_cuda or B == 0:  # (an empty batch launches nothing: the torch form returns the empty result on either device)
        return _class_maps_torch(pts, wts, img_hw, class_map_threshold, sigma, output_stride)
    out = torch.empty((B, Cn, h, w), dtype=torch.float32, device=pts.device)
    with torch.cuda.device(pts.device):
        L.check(L.lib().ph_render_class_maps(C.c_void_p(pts.data_ptr()), C.c_void_p(wts.data_ptr()), B, I, N, Cn, int(img_hw[0]), int(img_hw[1]), int(output_stride),
                                             float(sigma), float(class_map_threshold), C.c_void_p(out.data_ptr()), L.current_stream_ptr()))
    return out


def filter_oob_points(points: torch.Tensor, img_height: int, img_width: int) -> torch.Tensor:
    """A copy of ``points`` (..., 2) in which every point with a negative coordinate, ``x >= img_width`` or ``y >= img_height`` is NaN in
    both coordinates (``data/providers.py:38-69``: such a point would leave a partial blob on the edge of the target)."""
    x, y = points[..., 0], points[..., 1]
    oob = (x < 0) | (x >= img_width) | (y < 0) | (y >= img_height)
    return torch.where(oob.unsqueeze(-1), torch.full_like(points, float("nan")), points)


def _multiconfmaps(instances: torch.Tensor, img_hw, sigma: float, output_stride: int) -> torch.Tensor:
    if instances.is_cuda:
        return generate_multiconfmaps(instances, img_hw, sigma=sigma, output_stride=output_stride)
    pts = (instances.unsqueeze(-2) if instances.dim() == 3 else instances).to(torch.float32)
    if pts.shape[1] == 0:
        return torch.zeros((pts.shape[0], pts.shape[2], _grid(img_hw[0], output_stride), _grid(img_hw[1], output_stride)), dtype=torch.float32)
    return _gaussians(pts, img_hw, sigma, output_stride).amax(dim=1)


def _pafs(instances: torch.Tensor, img_hw, sigma: float, output_stride: int, edge_inds) -> torch.Tensor:
    """``generate_pafs`` for either device; the torch form states what ``render_pafs_kernel`` computes (csrc/train_kernels.hip)."""
    if instances.is_cuda:
        return generate_pafs(instances, img_hw, sigma=sigma, output_stride=output_stride, edge_inds=edge_inds)
    pts = instances.to(torch.float32)
    B, I, N, _ = pts.shape
    xv, yv = _grid_vectors(img_hw, output_stride, pts.device)
    e = torch.tensor([list(x) for x in edge_inds], dtype=torch.long).reshape(-1, 2)
    lim = torch.stack([xv[-1], yv[-1]])
    inside = ((pts > 0) & (pts < lim)).all(dim=-1).any(dim=-1)  # (B, I): an instance with no node strictly inside the grid is dropped
    src, dst = pts[:, :, e[:, 0]], pts[:, :, e[:, 1]]  # (B, I, E, 2)
    v = (dst - src)[..., None, None, :]  # (B, I, E, 1, 1, 2)
    grid = torch.stack(torch.meshgrid(xv, yv, indexing="xy"), dim=-1)  # (h, w, 2)
    r = grid - src[..., None, None, :]
    len2 = (v * v).sum(-1)
    t = ((r * v).sum(-1) / len2.clamp(min=1.0)).clamp(0.0, 1.0)
    off = t.unsqueeze(-1) * v - r
    d2 = (off * off).sum(-1)  # the SQUARED distance, which the reference feeds to its Gaussian as if it were the distance
    field = torch.exp(-(d2 * d2) / (2 * sigma**2)).unsqueeze(-1) * (v / len2.sqrt().unsqueeze(-1))
    field = torch.nan_to_num(field, nan=0.0) * inside[:, :, None, None, None, None]
    return field.sum(dim=1).permute(0, 1, 4, 2, 3).reshape(B, 2 * e.shape[0], yv.numel(), xv.numel())


_SEGMENTATION_TYPES = ("bottomup_segmentation", "semantic_segmentation", "centered_instance_segmentation")


class TargetGenerator:
    """The training targets of one model type, keyed by its head class names (what ``TrainingModule.training_step`` takes beside ``image``).

    ``head_config``: the model type's head config (``model_config.head_configs.<model_type>``); each head's own ``sigma`` and ``output_stride``
    are used.  ``anchor_ind``: node index of the centroid anchor (``centroid`` only).  ``__call__(instances, img_hw, class_inds, num_tracks)``:

    ====================== ================================================================================================================
    ``single_instance``    ``instances`` (B, N, 2) or (B, 1, N, 2)
    ``centroid``           ``instances`` (B, I, N, 2): ``generate_centroids`` then the one-channel maximum over the instances
    ``bottomup``           ``instances`` (B, I, N, 2): confidence maps and part-affinity fields
    ``multi_class_bottomup`` ``instances`` (B, I, N, 2), ``class_inds`` (B, I): confidence maps and class maps
    ``centered_instance``  ``instances`` (B, N, 2), already in crop coordinates: ``filter_oob_points`` then one Gaussian per node
    ``multi_class_topdown`` as ``centered_instance``, plus ``class_inds`` (B,) -> float one-hot rows for the class-vector head
    ====================== ================================================================================================================

    ``num_tracks`` defaults to the number of classes of the head config.  The tensors may live on the GPU (kernels) or the CPU (torch)."""

    def __init__(self, model_type: str, head_config, anchor_ind: Optional[int] = None, class_map_threshold: float = 0.2) -> None:
        from sleap_nn_amd.architectures.heads import get_head

        if model_type in _SEGMENTATION_TYPES:
            raise NotImplementedError(f"'{model_type}' targets (masks, centre maps, offsets) are not rendered here: use sleap_nn_amd.data.segmentation_maps.SegmentationTargetGenerator")
        self.model_type = model_type
        self.heads = {h.name: h for h in get_head(model_type, head_config)}
        self.anchor_ind = anchor_ind
        self.class_map_threshold = float(class_map_threshold)
        if model_type == "bottomup":
            names = self.heads["MultiInstanceConfmapsHead"].part_names
            self.edge_inds = [(names.index(a), names.index(b)) for a, b in self.heads["PartAffinityFieldsHead"].edges]

    @classmethod
    def from_training_config(cls, cfg_or_path, class_map_threshold: float = 0.2) -> "TargetGenerator":
        """From a sleap-nn training config (dict, YAML path or run directory): the non-empty entry of ``model_config.head_configs`` and, for
        ``anchor_part``, the node names of the first skeleton of ``data_config.skeletons`` (the confmaps head's ``part_names`` without one)."""
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
        if model_type in _SEGMENTATION_TYPES:
            return cls(model_type, heads[model_type])  # raises
        confmaps = heads[model_type].get("confmaps") or {}
        skels = (cfg.get("data_config") or {}).get("skeletons") or []
        skel = skels[0] if skels and isinstance(skels[0], dict) else {}
        names = [n["name"] if isinstance(n, dict) else str(n) for n in skel.get("nodes") or []] or list(confmaps.get("part_names") or [])
        anchor = confmaps.get("anchor_part")
        if anchor is not None and anchor not in names:
            raise ValueError(f"anchor_part '{anchor}' is not a node of the skeleton {names}")
        return cls(model_type, heads[model_type], names.index(anchor) if anchor is not None else None, class_map_threshold)

    def __call__(self, instances: torch.Tensor, img_hw: Tuple[int, int], class_inds: Optional[torch.Tensor] = None, num_tracks: Optional[int] = None) -> Dict[str, torch.Tensor]:
        H = self.heads
        mt = self.model_type

        def cm(name, fn, pts):
            return fn(pts, img_hw, sigma=H[name].sigma, output_stride=H[name].output_stride)

        if mt == "single_instance":
            return {"SingleInstanceConfmapsHead": cm("SingleInstanceConfmapsHead", generate_confmaps, instances)}
        if mt == "centroid":
            return {"CentroidConfmapsHead": cm("CentroidConfmapsHead", _multiconfmaps, generate_centroids(instances, self.anchor_ind))}
        if mt == "bottomup":
            paf = H["PartAffinityFieldsHead"]
            return {"MultiInstanceConfmapsHead": cm("MultiInstanceConfmapsHead", _multiconfmaps, instances),
                    "PartAffinityFieldsHead": _pafs(instances, img_hw, paf.sigma, paf.output_stride, self.edge_inds)}
        if mt == "multi_class_bottomup":
            if class_inds is None:
                raise ValueError("multi_class_bottomup targets need class_inds (B, I)")
            cmh = H["ClassMapsHead"]
            return {"MultiInstanceConfmapsHead": cm("MultiInstanceConfmapsHead", _multiconfmaps, instances),
                    "ClassMapsHead": generate_class_maps(instances, img_hw, class_inds, num_tracks if num_tracks is not None else len(cmh.classes),
                                                         class_map_threshold=self.class_map_threshold, sigma=cmh.sigma, output_stride=cmh.output_stride)}
        if instances.dim() != 3:
            raise ValueError(f"{mt} targets take one instance per sample, (B, N, 2) in crop coordinates; got {tuple(instances.shape)}")
        out = {"CenteredInstanceConfmapsHead": cm("CenteredInstanceConfmapsHead", generate_confmaps, filter_oob_points(instances, img_hw[0], img_hw[1]))}
        if mt == "multi_class_topdown":
            if class_inds is None:
                raise ValueError("multi_class_topdown targets need class_inds (B,)")
            n = num_tracks if num_tracks is not None else len(H["ClassVectorsHead"].classes)
            out["ClassVectorsHead"] = make_class_vectors(class_inds.to(instances.device), n).to(torch.float32)
        return out
