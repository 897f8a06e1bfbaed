"""Pose-estimation metrics on plain arrays and the epoch-end evaluation hook of the training loop.

Restates the arithmetic of ``sleap_nn/evaluation.py`` (``compute_instance_area`` :626-641, ``compute_oks`` :644-760,
``match_instances`` :763-856, ``compute_dists`` :904-939 and the ``Evaluator`` metrics ``voc_metrics`` :1253-1362,
``mOKS`` :1364-1367, ``distance_metrics`` :1369-1400, ``pck_metrics`` :1824-1862) without sleap-io objects: a frame is a
``(n_instances, n_nodes, 2)`` array with NaN for missing points, a prediction additionally carries one score per instance.
``EpochEndEvaluator`` is the counterpart of the per-batch collection in the LightningModules' ``validation_step``
(``training/lightning_modules.py:1099-1142``) and of ``training/callbacks.py:1263-1323``: predictions arrive in original image
space, ground truth is divided by the sample's ``eff_scale``; metrics are computed once per epoch on the host.
Host-side NumPy by design: a few hundred instances per epoch, nothing for a GPU to do.
"""
from __future__ import annotations

import warnings
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np


def compute_instance_area(points: np.ndarray) -> np.ndarray:
    """Bounding-box area of each instance's visible points (evaluation.py:626-641)."""
    pts = np.asarray(points)
    if pts.ndim == 2:
        pts = pts[None]
    return np.prod(np.nanmax(pts, axis=-2) - np.nanmin(pts, axis=-2), axis=-1)


def compute_oks(points_gt: np.ndarray, points_pr: np.ndarray, scale=None, stddev=0.025, use_cocoeval: bool = True) -> np.ndarray:
    """Object keypoint similarity of every (ground truth, prediction) pair -> ``(n_gt, n_pr)`` (evaluation.py:644-760)."""
    gt = np.asarray(points_gt, dtype=np.float64 if np.asarray(points_gt).dtype == np.float64 else np.asarray(points_gt).dtype)
    pr = np.asarray(points_pr)
    if gt.ndim == 2:
        gt = gt[None]
    if pr.ndim == 2:
        pr = pr[None]
    n_gt, n_nodes, _ = gt.shape
    area = compute_instance_area(gt) if scale is None else (np.full(n_gt, scale) if np.isscalar(scale) else np.asarray(scale))
    sd = np.full(n_nodes, stddev) if np.isscalar(stddev) else np.asarray(stddev)
    d2 = ((gt[:, None] - pr[None]) ** 2).sum(axis=-1)  # (n_gt, n_pr, n_nodes) squared distances
    if use_cocoeval:
        norm = ((2 * sd) ** 2)[None, None, :] * (2 * (area + np.spacing(1)))[:, None, None]
    else:
        norm = (sd**2)[None, None, :] * (2 * ((area + np.spacing(1)) ** 2))[:, None, None]
    d2[:, np.isnan(pr).any(axis=-1)] = np.inf  # a missing predicted point is a miss
    ks = np.exp(-(d2 / norm))
    missing_gt = np.isnan(gt).any(axis=-1)
    ks[np.broadcast_to(missing_gt[:, None, :], ks.shape)] = 0  # invisible ground truth does not count
    n_visible = (~missing_gt).astype("float32").sum(axis=-1, keepdims=True)
    return ks.sum(axis=-1) / n_visible


def match_instances(gt: np.ndarray, pr: np.ndarray, pr_scores: np.ndarray, stddev=0.025, scale=None, threshold: float = 0.0):
    """PASCAL-VOC style greedy matching inside one frame (evaluation.py:763-856): predictions in descending score order
    (stable), each takes the available ground-truth instance with the best OKS above ``threshold``.

    Returns ``(pairs, false_negatives)``: ``pairs`` = list of ``(gt index, prediction index, oks)``, ``false_negatives`` = the
    unmatched ground-truth indices."""
    gt = np.asarray(gt)
    pr = np.asarray(pr)
    available = list(range(len(gt)))
    pairs: List[Tuple[int, int, float]] = []
    if len(gt) == 0:
        return pairs, available
    for ip in np.argsort(-np.asarray(pr_scores, dtype=np.float64), kind="mergesort"):
        oks = compute_oks(gt[available], pr[ip : ip + 1], stddev=stddev, scale=scale)[:, 0]
        oks[oks <= threshold] = np.nan
        best = int(np.argsort(-oks, kind="mergesort")[0])
        if np.isnan(oks[best]):
            continue
        pairs.append((available.pop(best), int(ip), float(oks[best])))
        if not available:
            break
    return pairs, available


class Evaluator:
    """Metrics over matched frames (evaluation.py:942-1016 restricted to the pose metrics of ``evaluate`` :1893-1941)."""

    def __init__(self, frames_gt: Sequence[np.ndarray], frames_pr: Sequence[np.ndarray], frames_pr_scores: Sequence[np.ndarray], oks_stddev: float = 0.025,
                 oks_scale: Optional[float] = None, match_threshold: float = 0.0) -> None:
        self.pair_oks: List[float] = []
        self.pair_scores: List[float] = []
        dists = []
        self.n_false_negatives = 0
        for g, p, s in zip(frames_gt, frames_pr, frames_pr_scores):
            g, p, s = np.asarray(g), np.asarray(p), np.asarray(s)
            keep_g = ~np.isnan(g).all(axis=(1, 2)) if len(g) else np.zeros(0, bool)
            keep_p = ~np.isnan(p).all(axis=(1, 2)) if len(p) else np.zeros(0, bool)
            g, p, s = g[keep_g], p[keep_p], s[keep_p]
            if len(g) == 0 or len(p) == 0:  # find_frame_pairs only pairs frames present on both sides (evaluation.py:558-623)
                continue
            pairs, fn = match_instances(g, p, s, stddev=oks_stddev, scale=oks_scale, threshold=match_threshold)
            self.n_false_negatives += len(fn)
            for ig, ip, oks in pairs:
                self.pair_oks.append(oks)
                self.pair_scores.append(float(s[ip]))
                dists.append(np.linalg.norm(p[ip] - g[ig], axis=-1))
        self.dists = np.array(dists)

    def mOKS(self) -> Dict[str, float]:
        o = np.array(self.pair_oks)
        return {"mOKS": float(o.mean()) if o.size else float("nan")}

    def voc_metrics(self, match_score_thresholds=np.linspace(0.5, 0.95, 10), recall_thresholds=np.linspace(0, 1, 101)) -> Dict[str, object]:
        name = "oks_voc"
        order = np.argsort(-np.array(self.pair_scores), kind="mergesort")
        match_scores = np.array(self.pair_oks)[order]
        npig = len(self.pair_oks) + self.n_false_negatives
        if match_scores.size == 0:
            return {f"{name}.{k}": 0 for k in ("match_score_thresholds", "recall_thresholds", "match_scores", "precisions", "recalls", "AP", "AR", "mAP", "mAR")}
        precisions, recalls = [], []
        for thr in match_score_thresholds:
            tp = np.cumsum(match_scores >= thr)
            fp = np.cumsum(match_scores < thr)
            rc = tp / npig
            pr = tp / (fp + tp + np.spacing(1))
            for i in range(len(pr) - 1, 0, -1):  # monotone non-increasing precision envelope
                if pr[i] > pr[i - 1]:
                    pr[i - 1] = pr[i]
            inds = np.searchsorted(rc, recall_thresholds, side="left")
            prec = np.zeros(inds.shape)
            ok = inds < len(pr)
            prec[ok] = pr[inds[ok]]
            precisions.append(prec)
            recalls.append(rc[-1])
        precisions, recalls = np.array(precisions), np.array(recalls)
        return {f"{name}.match_score_thresholds": match_score_thresholds, f"{name}.recall_thresholds": recall_thresholds, f"{name}.match_scores": match_scores,
                f"{name}.precisions": precisions, f"{name}.recalls": recalls, f"{name}.AP": precisions.mean(axis=1), f"{name}.AR": recalls,
                f"{name}.mAP": precisions.mean(), f"{name}.mAR": recalls.mean()}

    def distance_metrics(self) -> Dict[str, object]:
        d = self.dists
        out = {"dists": d, "avg": float(np.nanmean(d)) if d.size and not np.all(np.isnan(d)) else float("nan")}
        ok = ~np.isnan(d) if d.size else np.zeros(0, bool)
        for p in (50, 75, 90, 95, 99):
            out[f"p{p}"] = float(np.percentile(d[ok], p)) if ok.any() else float("nan")
        return out

    def pck_metrics(self, thresholds=np.linspace(1, 10, 10)) -> Dict[str, object]:
        d = np.copy(self.dists)
        if d.size == 0:
            return {"thresholds": thresholds, "pcks": np.zeros((0, 0, len(thresholds)), bool), "mPCK_parts": np.array([]), "mPCK": float("nan"), "PCK@5": float("nan"), "PCK@10": float("nan")}
        d[np.isnan(d)] = np.inf
        pcks = d[..., None] < np.reshape(thresholds, (1, 1, -1))
        parts = pcks.mean(axis=0).mean(axis=-1)
        return {"thresholds": thresholds, "pcks": pcks, "mPCK_parts": parts, "mPCK": float(parts.mean()),
                "PCK@5": float(pcks[:, :, int(np.argmin(np.abs(thresholds - 5)))].mean()), "PCK@10": float(pcks[:, :, int(np.argmin(np.abs(thresholds - 10)))].mean())}

    def evaluate(self) -> Dict[str, object]:
        return {"voc_metrics": self.voc_metrics(), "mOKS": self.mOKS(), "distance_metrics": self.distance_metrics(), "pck_metrics": self.pck_metrics()}


class EpochEndEvaluator:
    """Collect (prediction, ground truth) per validation sample, evaluate at the end of the epoch.

    ``add_batch`` takes an ``Outputs`` of an inference layer (keypoints already in original image space) and the batch's
    ground-truth instances in PREPROCESSED space with their ``eff_scale`` and ``num_instances``
    (lightning_modules.py:1112-1141); ``compute`` returns the metrics dictionary and clears the lists
    (callbacks.py:1263-1323; only every ``eval_frequency``-th epoch evaluates)."""

    def __init__(self, oks_stddev: float = 0.025, oks_scale: Optional[float] = None, eval_frequency: int = 1) -> None:
        self.oks_stddev, self.oks_scale, self.eval_frequency = oks_stddev, oks_scale, int(eval_frequency)
        self._pred: List[np.ndarray] = []
        self._score: List[np.ndarray] = []
        self._gt: List[np.ndarray] = []

    def add_batch(self, outputs, gt_instances, eff_scale, num_instances) -> None:
        kp = np.asarray(outputs.pred_keypoints)
        vals = np.asarray(outputs.pred_peak_values)
        gt = np.asarray(gt_instances, dtype=np.float32)
        eff = np.asarray(eff_scale, dtype=np.float32).reshape(-1)
        for i in range(kp.shape[0]):
            k, v = kp[i], vals[i]
            if k.ndim == 2:  # single instance: (n_nodes, 2)
                k, v = k[None], v[None]
            g = gt[i]
            if g.ndim == 4:
                g = g[0]  # the n_samples axis
            self._pred.append(k)
            with warnings.catch_warnings():
                warnings.simplefilter("ignore", RuntimeWarning)  # an all-NaN (padding) instance: nanmean -> NaN, dropped by the Evaluator
                self._score.append(np.nanmean(v, axis=-1))  # instance score = mean peak value (callbacks.py:1366-1370)
            self._gt.append((g / eff[i])[: int(num_instances[i])])

    def compute(self, epoch: int = 0) -> Optional[Dict[str, object]]:
        out = None
        if (epoch + 1) % self.eval_frequency == 0 and self._pred:
            out = Evaluator(self._gt, self._pred, self._score, self.oks_stddev, self.oks_scale).evaluate()
        self._pred, self._score, self._gt = [], [], []
        return out


# ---- segmentation masks ----------------------------------------------------------------------------------------------------------------
#
# Restates ``_mask_iou`` :120-143, ``match_masks`` :161-219, ``_percentile_size_edges`` :306-320, ``_size_mask`` :323-336, ``_align_pair``
# :339-349, ``_mask_pair_stats`` :352-372, ``_mask_to_boundary`` :375-393, ``_boundary_iou`` :396-409, ``_ap_from_pr`` :465-506 and the
# ``Evaluator`` methods ``_process_frames_mask`` :1134-1202, ``_process_frames_semantic`` :1204-1237, ``mask_metrics`` :1456-1552,
# ``semantic_metrics`` :1554-1585, ``_fragmentation_counts`` :1587-1609, ``_mask_per_size_stats`` :1611-1663, ``_match_masks_coco``
# :1665-1715 and ``mask_voc_metrics`` :1717-1822 on mask BATCHES instead of sleap-io frames.  The per-pixel work -- the intersection count
# of every (prediction, ground truth) pair with every mask's area, and the boundary regions -- runs in ``ph_mask_pair_stats`` /
# ``ph_mask_boundary`` (csrc/eval_kernels.hip) for tensors on the GPU and in NumPy, to the identical integer contract, for CPU tensors
# and arrays; everything after the integer tables (IoU, matching, AP) is float64 NumPy on a few numbers per frame either way.
# clDice (``mask_cldice`` :427-462) is not built: ``mean_cldice`` is NaN, what the reference reports without scikit-image.

MASK_IOU_THRESHOLDS = np.linspace(0.5, 0.95, 10)
_SIZE_KEYS = ("small", "medium", "large")
COCO_SIZE_EDGES = np.array([32**2, 96**2], dtype=float)
DEFAULT_SIZE_PERCENTILES = (100.0 / 3.0, 200.0 / 3.0)
MAX_DEVICE_MASKS = 64  # ph_mask_pair_stats: one bit of a 64-bit membership word per mask; larger sets take the host path
_MAX_FRAMES_PER_CALL = 65535  # ph_mask_pair_stats: frames ride on the grid's y axis


def _percentile_size_edges(gt_areas, percentiles=DEFAULT_SIZE_PERCENTILES) -> np.ndarray:
    g = np.asarray(gt_areas, dtype=float)
    g = g[~np.isnan(g)]
    if g.size == 0:
        return np.array([np.nan, np.nan])
    return np.percentile(g, list(percentiles))


def _size_mask(areas, bucket_idx: int, edges) -> np.ndarray:
    """Half-open buckets ``(-inf, e0)``, ``[e0, e1)``, ``[e1, inf)``; NaN areas and NaN edges fall in none."""
    areas = np.asarray(areas, dtype=float)
    lo = -np.inf if bucket_idx == 0 else edges[bucket_idx - 1]
    hi = np.inf if bucket_idx >= len(edges) else edges[bucket_idx]
    with np.errstate(invalid="ignore"):
        return (areas >= lo) & (areas < hi)


def _ap_from_pr(scores, is_tp, npig: int, recall_thresholds) -> Tuple[float, float]:
    """Average precision and final recall of score-ranked TP / FP flags, 101-point interpolated (evaluation.py:465-506)."""
    if npig <= 0:
        return np.nan, np.nan
    scores = np.asarray(scores, dtype=float)
    is_tp = np.asarray(is_tp, dtype=bool)
    if scores.size == 0:
        return 0.0, 0.0
    is_tp = is_tp[np.argsort(-scores, kind="mergesort")]
    tp = np.cumsum(is_tp)
    fp = np.cumsum(~is_tp)
    rc = tp / npig
    pr = tp / np.maximum(tp + fp, np.spacing(1))
    for i in range(pr.size - 1, 0, -1):
        if pr[i] > pr[i - 1]:
            pr[i - 1] = pr[i]
    inds = np.searchsorted(rc, recall_thresholds, side="left")
    precision = np.zeros(np.shape(recall_thresholds))
    valid = inds < pr.size
    precision[valid] = pr[inds[valid]]
    return float(precision.mean()), float(rc[-1])


def _on_device(x) -> bool:
    return hasattr(x, "is_cuda") and bool(x.is_cuda)


def _to_numpy(x) -> np.ndarray:
    return x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x)


def _counts(n, B: int, full: int) -> np.ndarray:
    if n is None:
        return np.full(B, full, dtype=np.int64)
    n = _to_numpy(n).astype(np.int64).reshape(-1)
    if n.shape[0] != B:
        raise ValueError(f"expected {B} counts, got {n.shape[0]}")
    return np.clip(n, 0, full)


def _pred_layout(pred, n_pred):
    """``(is_stack, B, P, ph, pw)`` of a prediction batch: a stack (B, P, ph, pw) or a label map (B, ph, pw), whose P is the largest count."""
    if pred.ndim == 4:
        return True, pred.shape[0], pred.shape[1], pred.shape[2], pred.shape[3]
    if pred.ndim != 3:
        raise ValueError(f"prediction must be a mask stack (B, P, h, w) or a label map (B, h, w), got shape {tuple(pred.shape)}")
    if n_pred is None:
        raise ValueError("a label map needs n_pred")
    return False, pred.shape[0], int(_to_numpy(n_pred).max(initial=0)), pred.shape[1], pred.shape[2]


def _pair_tables_host(pred: np.ndarray, gt: np.ndarray, n_pred: np.ndarray, n_gt: np.ndarray, s: int, is_stack: bool, P: int):
    """The contract of ``ph_mask_pair_stats`` in NumPy: per prediction, its pixels' indices gather the ground-truth stack."""
    B, G, H, W = gt.shape
    ph, pw = pred.shape[-2:]
    Hc, Wc = max(H, ph * s), max(W, pw * s)
    inter = np.zeros((B, P, G), np.int32)
    pa = np.zeros((B, P), np.int32)
    ga = np.zeros((B, G), np.int32)
    for b in range(B):
        ng, npb = int(n_gt[b]), int(n_pred[b])
        gm = np.zeros((ng, Hc, Wc), bool)
        gm[:, :H, :W] = gt[b, :ng] != 0
        gm = gm.reshape(ng, Hc * Wc)
        ga[b, :ng] = gm.sum(axis=1)
        if is_stack:
            cells = pred[b, :npb] != 0
        else:
            cells = pred[b][None] == np.arange(npb, dtype=np.int64)[:, None, None]
        for p in range(npb):
            canvas = np.zeros((Hc, Wc), bool)
            canvas[: ph * s, : pw * s] = np.repeat(np.repeat(cells[p], s, axis=0), s, axis=1) if s > 1 else cells[p]
            idx = np.flatnonzero(canvas)
            pa[b, p] = idx.size
            if idx.size and ng:
                inter[b, p, :ng] = gm[:, idx].sum(axis=1)
    return inter, pa, ga


def _pair_tables_device(pred, gt, n_pred: np.ndarray, n_gt: np.ndarray, s: int, is_stack: bool, P: int):
    """``ph_mask_pair_stats`` on the current stream; int32 device tensors ``(B, P, G)``, ``(B, P)``, ``(B, G)``.  No host synchronisation."""
    import ctypes as C

    import torch

    from sleap_nn_amd import _lib as L

    lib = L.lib()
    B, G, H, W = gt.shape
    ph, pw = pred.shape[-2:]
    dev = gt.device
    byte = lambda t: (t.view(torch.uint8) if t.dtype == torch.bool else t.to(torch.uint8)).contiguous()
    gt = byte(gt)
    if is_stack:
        pred, form = byte(pred), 0
    else:
        if pred.dtype not in (torch.int8, torch.int16, torch.int32):
            pred = pred.to(torch.int32)
        pred, form = pred.contiguous(), pred.element_size()
    p = lambda t: C.c_void_p(t.data_ptr())
    with torch.cuda.device(dev):
        counts = torch.from_numpy(np.stack([n_pred, n_gt]).astype(np.int32)).to(dev)
        out = torch.empty(B * (P * G + P + G), dtype=torch.int32, device=dev)
        inter, pa, ga = out[: B * P * G].view(B, P, G), out[B * P * G : B * (P * G + P)].view(B, P), out[B * (P * G + P) :].view(B, G)
        st = L.current_stream_ptr()
        for b0 in range(0, B, _MAX_FRAMES_PER_CALL):
            b1 = min(B, b0 + _MAX_FRAMES_PER_CALL)
            L.check(lib.ph_mask_pair_stats(p(pred[b0:b1]), form, P, ph, pw, int(s), p(gt[b0:b1]), G, H, W, b1 - b0, p(counts[0, b0:b1]), p(counts[1, b0:b1]),
                                           p(inter[b0:b1]), p(pa[b0:b1]), p(ga[b0:b1]), st))
    return inter, pa, ga


def _from_outputs(pred, gt, n_pred, pred_stride: int):
    """``(pred, n_pred, pred_stride, scores)`` of a prediction batch given as an inference ``Outputs``; anything else passes through with ``scores=None``.

    With ``pred_mask_stack`` / ``pred_mask_counts`` (top-down segmentation, ``place_masks=True``) the device stack is the prediction as it is: stack form,
    stride 1, no host round trip.  Otherwise the host ``pred_masks`` entries -- any ``offset``, any ``scale`` -- are decoded into a stack at the ground
    truth's frame size by ``place_crop_masks``' host implementation (``ops.segmentation.stack_pred_masks``) and follow ``gt`` onto its device."""
    if not hasattr(pred, "pred_masks"):
        return pred, n_pred, pred_stride, None
    if pred.pred_masks is None:
        raise ValueError("these Outputs carry no pred_masks")
    scores = [np.array([d["score"] for d in frame], dtype=float) for frame in pred.pred_masks]
    if getattr(pred, "pred_mask_stack", None) is not None:
        stack = pred.pred_mask_stack
        if _on_device(gt) and not _on_device(stack):
            stack = stack.to(gt.device)
        return stack, pred.pred_mask_counts, 1, scores
    from sleap_nn_amd.inference.ops.segmentation import stack_pred_masks

    stack, counts = stack_pred_masks(pred.pred_masks, gt.shape[-2:])
    if hasattr(gt, "device"):
        import torch

        stack = torch.from_numpy(stack).to(gt.device)
    return stack, counts, 1, scores


def mask_pair_tables(pred, gt, n_pred=None, n_gt=None, pred_stride: int = 1):
    """Integer tables of a batch: ``inter (B, P, G)``, ``pred_area (B, P)``, ``gt_area (B, G)``, int32, slots beyond a frame's counts 0.

    ``gt``: ``(B, G, H, W)``, nonzero = foreground.  ``pred``: a stack ``(B, P, ph, pw)`` or a label map ``(B, ph, pw)`` of signed
    integers (``-1`` = background, labels in ``[0, n_pred)``), read at cell ``(y // pred_stride, x // pred_stride)`` on the top-left
    aligned canvas ``max(H, ph * s) x max(W, pw * s)`` (``_align_pair``).  Tensors on the GPU with at most 64 masks per side come back
    as device tensors from ``ph_mask_pair_stats`` without a host synchronisation; everything else is NumPy on the host.  ``pred`` may also be an
    inference ``Outputs`` with masks (``_from_outputs``)."""
    pred, n_pred, pred_stride, _ = _from_outputs(pred, gt, n_pred, pred_stride)
    s = int(pred_stride)
    if s < 1:
        raise ValueError(f"pred_stride must be >= 1, got {pred_stride}")
    if gt.ndim != 4:
        raise ValueError(f"ground truth must be (B, G, H, W), got shape {tuple(gt.shape)}")
    is_stack, B, P, ph, pw = _pred_layout(pred, n_pred)
    if gt.shape[0] != B:
        raise ValueError(f"{B} prediction frames, {gt.shape[0]} ground-truth frames")
    G = gt.shape[1]
    n_pred, n_gt = _counts(n_pred, B, P), _counts(n_gt, B, G)
    if _on_device(pred) != _on_device(gt):
        raise ValueError("prediction and ground truth must both be on the GPU or both on the host")
    if _on_device(gt) and 1 <= P <= MAX_DEVICE_MASKS and 1 <= G <= MAX_DEVICE_MASKS and B > 0 and min(ph, pw, gt.shape[2], gt.shape[3]) > 0:
        return _pair_tables_device(pred, gt, n_pred, n_gt, s, is_stack, P)
    return _pair_tables_host(_to_numpy(pred), _to_numpy(gt), n_pred, n_gt, s, is_stack, P)


def _iou_from_tables(inter: np.ndarray, pa: np.ndarray, ga: np.ndarray) -> np.ndarray:
    inter = inter.astype(np.int64)
    union = pa.astype(np.int64)[:, None] + ga.astype(np.int64)[None, :] - inter
    iou = np.ones(inter.shape, dtype=np.float64)  # an empty union: two empty masks are identical (_mask_iou)
    np.divide(inter, union, out=iou, where=union != 0)
    return iou


def mask_pair_stats(pred, gt, n_pred=None, n_gt=None, pred_stride: int = 1):
    """Per frame ``(iou (n_pred, n_gt) float64, inter int64, pred_area int64 (n_pred,), gt_area int64 (n_gt,))`` of ``mask_pair_tables``'
    batch: ``iou = inter / (pred_area + gt_area - inter)``, 1.0 where the union is empty (``_mask_pair_stats`` + the areas)."""
    pred, n_pred, pred_stride, _ = _from_outputs(pred, gt, n_pred, pred_stride)
    is_stack, B, P, _, _ = _pred_layout(pred, n_pred)
    n_pred, n_gt = _counts(n_pred, B, P), _counts(n_gt, B, gt.shape[1])
    inter, pa, ga = (_to_numpy(t) for t in mask_pair_tables(pred, gt, n_pred, n_gt, pred_stride))
    out = []
    for b in range(B):
        i, a, g = inter[b, : n_pred[b], : n_gt[b]].astype(np.int64), pa[b, : n_pred[b]].astype(np.int64), ga[b, : n_gt[b]].astype(np.int64)
        out.append((_iou_from_tables(i, a, g), i, a, g))
    return out


def match_masks(iou, min_iou: float = 0.5):
    """Hungarian matching that maximises the total IoU of an ``(n_pred, n_gt)`` matrix; pairs below ``min_iou`` are dropped.

    Returns ``(matched_pred, matched_gt, unmatched_pred, unmatched_gt, matched_ious)`` (evaluation.py:161-219)."""
    from scipy.optimize import linear_sum_assignment

    iou = np.asarray(iou, dtype=float)
    n_pred, n_gt = iou.shape
    empty = np.array([], dtype=int)
    if n_pred == 0 and n_gt == 0:
        return empty, empty, empty, empty, np.array([])
    if n_pred == 0:
        return empty, empty, empty, np.arange(n_gt), np.array([])
    if n_gt == 0:
        return empty, empty, np.arange(n_pred), empty, np.array([])
    rows, cols = linear_sum_assignment(-iou)
    keep = iou[rows, cols] >= min_iou
    mp, mg = rows[keep].astype(int), cols[keep].astype(int)
    return (mp, mg, np.array(sorted(set(range(n_pred)) - set(mp.tolist())), dtype=int), np.array(sorted(set(range(n_gt)) - set(mg.tolist())), dtype=int),
            iou[mp, mg].astype(float))


def boundary_width(h: int, w: int, dilation_ratio: float = 0.02) -> int:
    """``d`` of ``_mask_to_boundary``: 2 % of the image diagonal, rounded, at least 1."""
    return max(1, int(round(dilation_ratio * float(np.sqrt(h * h + w * w)))))


def mask_boundary(masks, d: Optional[int] = None):
    """Boundary regions of ``masks (N, H, W)``: ``mask AND NOT eroded`` where a pixel is eroded exactly when it lies at least ``d`` from every
    image edge and its ``(2d + 1) x (2d + 1)`` window is all foreground (``_mask_to_boundary``: ``d`` 3x3 erosions behind a one-pixel zero border).
    uint8 device tensor from ``ph_mask_boundary`` for a tensor on the GPU, NumPy bool array otherwise."""
    N, H, W = masks.shape
    d = boundary_width(H, W) if d is None else int(d)
    if d < 1:
        raise ValueError(f"d must be >= 1, got {d}")
    if _on_device(masks) and N > 0 and H > 0 and W > 0:
        import ctypes as C

        import torch

        from sleap_nn_amd import _lib as L

        lib = L.lib()
        m = (masks.view(torch.uint8) if masks.dtype == torch.bool else masks.to(torch.uint8)).contiguous()
        with torch.cuda.device(m.device):
            out = torch.empty_like(m)
            need = int(lib.ph_mask_boundary_scratch_bytes(N, H, W))
            scratch = torch.empty((need + 1) // 2, dtype=torch.int16, device=m.device)
            L.check(lib.ph_mask_boundary(C.c_void_p(m.data_ptr()), N, H, W, d, C.c_void_p(out.data_ptr()), C.c_void_p(scratch.data_ptr()), need, L.current_stream_ptr()))
        return out
    m = _to_numpy(masks) != 0
    eroded = np.zeros(m.shape, bool)
    k = 2 * d + 1
    if H >= k and W >= k:  # window sums from a summed-area table: all integers
        sat = np.zeros((N, H + 1, W + 1), np.int64)
        sat[:, 1:, 1:] = m.cumsum(axis=1, dtype=np.int64).cumsum(axis=2)
        eroded[:, d : H - d, d : W - d] = (sat[:, k:, k:] - sat[:, :-k, k:] - sat[:, k:, :-k] + sat[:, :-k, :-k]) == k * k
    return m & ~eroded


def _align_stack(x, Hc: int, Wc: int):
    """Top-left align a stack ``(N, h, w)`` on an ``Hc x Wc`` canvas (``_align_pair``)."""
    if tuple(x.shape[-2:]) == (Hc, Wc):
        return x
    if _on_device(x):
        import torch

        return torch.nn.functional.pad(x, (0, Wc - x.shape[-1], 0, Hc - x.shape[-2]))
    out = np.zeros(x.shape[:-2] + (Hc, Wc), x.dtype)
    out[..., : x.shape[-2], : x.shape[-1]] = x
    return out


def boundary_iou(pred, gt, dilation_ratio: float = 0.02) -> np.ndarray:
    """Boundary IoU (Cheng et al. 2021) of aligned pairs ``pred (N, h, w)`` / ``gt (N, H, W)`` -> float64 ``(N,)`` (``_boundary_iou``): both
    stacks on their common top-left aligned canvas, ``d`` from its diagonal, IoU of the two boundary regions, 1.0 when both are empty.
    On the GPU: ``ph_mask_boundary`` over both stacks at once, then ``ph_mask_pair_stats`` with one mask per side and one frame per pair."""
    N = pred.shape[0]
    if N == 0:
        return np.zeros(0, np.float64)
    if gt.shape[0] != N:
        raise ValueError(f"{N} predicted masks, {gt.shape[0]} ground-truth masks")
    dev = _on_device(pred) and _on_device(gt)
    if dev:
        import torch

        pred, gt = (t.view(torch.uint8) if t.dtype == torch.bool else (t != 0).view(torch.uint8) for t in (pred, gt))
    else:
        pred, gt = _to_numpy(pred) != 0, _to_numpy(gt) != 0
    Hc, Wc = max(pred.shape[1], gt.shape[1]), max(pred.shape[2], gt.shape[2])
    d = boundary_width(Hc, Wc, dilation_ratio)
    pred, gt = _align_stack(pred, Hc, Wc), _align_stack(gt, Hc, Wc)
    if dev:
        both = mask_boundary(torch.cat([pred, gt]), d)
        bp, bg = both[:N, None], both[N:, None]
    else:
        bp, bg = mask_boundary(pred, d)[:, None], mask_boundary(gt, d)[:, None]
    inter, pa, ga = (_to_numpy(t).astype(np.int64).reshape(N) for t in mask_pair_tables(bp, bg))
    union = pa + ga - inter
    out = np.ones(N, np.float64)
    np.divide(inter, union, out=out, where=union != 0)
    return out


def _upsample(x, s: int):
    if s == 1:
        return x
    if _on_device(x):
        return x.repeat_interleave(s, dim=-2).repeat_interleave(s, dim=-1)
    return np.repeat(np.repeat(x, s, axis=-2), s, axis=-1)


class MaskEvaluator:
    """Instance-mask metrics over batches of frames (``match_method="mask"``): ``add_batch`` reduces a batch to its per-frame tables (IoU,
    intersections, areas, scores) and the boundary IoUs of its matched pairs -- no mask is kept -- and ``mask_metrics`` / ``mask_voc_metrics``
    evaluate everything added so far."""

    def __init__(self, match_threshold: float = 0.5) -> None:
        self.match_threshold = match_threshold
        self.reset()

    def reset(self) -> None:
        self._frames: List[Dict[str, np.ndarray]] = []
        self._ious: List[float] = []
        self._tp_gt_area: List[float] = []
        self._boundary_ious: List[float] = []
        self.n_fp = 0
        self.n_fn = 0

    def __len__(self) -> int:
        return len(self._frames)

    def add_batch(self, pred, pred_scores, gt, n_pred=None, n_gt=None, pred_stride: int = 1) -> None:
        """``pred`` / ``gt`` / counts / stride as in ``mask_pair_tables``; ``pred_scores (B, P)`` (or one array per frame), ``None`` = 1.0 each (for an
        ``Outputs``: its entries' scores)."""
        pred, n_pred, pred_stride, own_scores = _from_outputs(pred, gt, n_pred, pred_stride)
        if pred_scores is None:
            pred_scores = own_scores
        is_stack, B, P, _, _ = _pred_layout(pred, n_pred)
        n_pred, n_gt = _counts(n_pred, B, P), _counts(n_gt, B, gt.shape[1])
        s = int(pred_stride)
        pairs_b, pairs_p, pairs_g = [], [], []
        for b, (iou, inter, pa, ga) in enumerate(mask_pair_stats(pred, gt, n_pred, n_gt, s)):
            sc = np.ones(n_pred[b]) if pred_scores is None else _to_numpy(pred_scores[b]).astype(float).reshape(-1)[: n_pred[b]]
            self._frames.append({"iou": iou, "inter": inter, "gt_areas": ga.astype(float), "pred_areas": pa.astype(float), "pred_scores": sc})
            mp, mg, up, ug, mi = match_masks(iou, self.match_threshold)
            self._ious.extend(float(v) for v in mi)
            self._tp_gt_area.extend(float(ga[g]) for g in mg)
            self.n_fp += len(up)
            self.n_fn += len(ug)
            pairs_b.extend([b] * len(mp))
            pairs_p.extend(int(v) for v in mp)
            pairs_g.extend(int(v) for v in mg)
        if not pairs_b:
            return
        if _on_device(gt):
            import torch

            ib, ip, ig = (torch.as_tensor(v, dtype=torch.long, device=gt.device) for v in (pairs_b, pairs_p, pairs_g))
            pm = pred[ib, ip] != 0 if is_stack else pred[ib] == ip[:, None, None].to(pred.dtype)
        else:
            pred, gt = _to_numpy(pred), _to_numpy(gt)
            ib, ip, ig = (np.asarray(v, dtype=np.int64) for v in (pairs_b, pairs_p, pairs_g))
            pm = pred[ib, ip] != 0 if is_stack else pred[ib] == ip[:, None, None]
        self._boundary_ious.extend(float(v) for v in boundary_iou(_upsample(pm, s), gt[ib, ig] != 0))

    # -- mask_metrics ------------------------------------------------------------------------------------------------------------------

    def _fragmentation_counts(self, overlap_frac: float = 0.1) -> Tuple[int, int]:
        over = under = 0
        for f in self._frames:
            inter = f["inter"]
            if inter.shape[0] == 0 or inter.shape[1] == 0:
                continue
            covers = inter / np.maximum(f["gt_areas"][None, :], 1.0) >= overlap_frac
            over += int(np.count_nonzero(covers.sum(axis=0) >= 2))  # a ground-truth mask split over predictions
            under += int(np.count_nonzero(covers.sum(axis=1) >= 2))  # a prediction that merges ground-truth masks
        return over, under

    def _gt_areas_all(self) -> np.ndarray:
        return np.array([a for f in self._frames for a in f["gt_areas"]], dtype=float)

    @staticmethod
    def _per_size_breakdown(gt_areas_all, tp_iou, tp_gt_area, edges) -> dict:
        out = {"edges": [float(e) for e in edges]}
        for idx, bucket in enumerate(_SIZE_KEYS):
            in_gt = _size_mask(gt_areas_all, idx, edges)
            in_tp = _size_mask(tp_gt_area, idx, edges) if tp_gt_area.size else np.array([], dtype=bool)
            out[bucket] = {"n_gt": int(np.count_nonzero(in_gt)), "n_tp": int(np.count_nonzero(in_tp)),
                           "mean_iou": float(np.mean(tp_iou[in_tp])) if np.any(in_tp) else np.nan}
        return out

    def _mask_per_size_stats(self) -> dict:
        gt_areas_all = self._gt_areas_all()
        tp_iou, tp_gt_area = np.asarray(self._ious, dtype=float), np.asarray(self._tp_gt_area, dtype=float)
        out = self._per_size_breakdown(gt_areas_all, tp_iou, tp_gt_area, _percentile_size_edges(gt_areas_all))
        out["scheme"] = "percentile"
        out["coco"] = self._per_size_breakdown(gt_areas_all, tp_iou, tp_gt_area, COCO_SIZE_EDGES)
        return out

    def mask_metrics(self) -> Dict[str, object]:
        ious = np.asarray(self._ious, dtype=float)
        n_tp, n_fp, n_fn = int(ious.size), self.n_fp, self.n_fn
        over, under = self._fragmentation_counts()
        r = {"mean_iou": np.nan, "min": np.nan, "max": np.nan, "p25": np.nan, "p50": np.nan, "p75": np.nan, "mean_iou_all_gt": np.nan, "pq": np.nan, "sq": np.nan,
             "rq": np.nan, "mean_boundary_iou": np.nan, "mean_cldice": np.nan, "oversegmentation": over, "undersegmentation": under,
             "per_size": self._mask_per_size_stats(), "n_matched": n_tp, "n_fp": n_fp, "n_fn": n_fn, "ious": ious}
        if ious.size:
            r["mean_iou"], r["min"], r["max"] = float(np.mean(ious)), float(np.min(ious)), float(np.max(ious))
            for ptile in (25, 50, 75):
                r[f"p{ptile}"] = float(np.percentile(ious, ptile))
        if self._boundary_ious:
            r["mean_boundary_iou"] = float(np.mean(np.array(self._boundary_ious, dtype=float)))
        iou_sum = float(np.sum(ious)) if ious.size else 0.0
        if n_tp + n_fn > 0:
            r["mean_iou_all_gt"] = iou_sum / (n_tp + n_fn)
        pq_denom = n_tp + 0.5 * n_fp + 0.5 * n_fn
        if pq_denom > 0:
            r["sq"], r["rq"], r["pq"] = r["mean_iou"], n_tp / pq_denom, iou_sum / pq_denom
        return r

    # -- mask_voc_metrics --------------------------------------------------------------------------------------------------------------

    def _match_masks_coco(self, iou_threshold: float):
        """Greedy, score-ranked (stable) matching per frame at one threshold -> flat ``(scores, matched, matched_gt_area, pred_area)``."""
        scores, matched, matched_gt_area, pred_area = [], [], [], []
        for f in self._frames:
            iou, pred_scores, gt_areas, pred_areas = f["iou"], f["pred_scores"], f["gt_areas"], f["pred_areas"]
            n_pred, n_gt = iou.shape
            order = np.argsort(-pred_scores, kind="mergesort") if n_pred else np.array([], dtype=int)
            taken = np.zeros(n_gt, dtype=bool)
            for p in order:
                scores.append(float(pred_scores[p]))
                pred_area.append(float(pred_areas[p]))
                if n_gt == 0:
                    matched.append(False)
                    matched_gt_area.append(np.nan)
                    continue
                row = iou[p].copy()
                row[taken] = -1.0
                g = int(np.argmax(row))
                if row[g] >= iou_threshold:
                    taken[g] = True
                    matched.append(True)
                    matched_gt_area.append(float(gt_areas[g]))
                else:
                    matched.append(False)
                    matched_gt_area.append(np.nan)
        return np.array(scores, dtype=float), np.array(matched, dtype=bool), np.array(matched_gt_area, dtype=float), np.array(pred_area, dtype=float)

    def mask_voc_metrics(self, iou_thresholds=MASK_IOU_THRESHOLDS, recall_thresholds=np.linspace(0, 1, 101), size_percentiles=DEFAULT_SIZE_PERCENTILES) -> Dict[str, object]:
        iou_thresholds = np.asarray(iou_thresholds, dtype=float)
        recall_thresholds = np.asarray(recall_thresholds, dtype=float)
        gt_areas_all = self._gt_areas_all()
        npig = int(gt_areas_all.size)
        schemes = {"percentile": _percentile_size_edges(gt_areas_all, size_percentiles), "coco": COCO_SIZE_EDGES}
        n_gt_size = {name: [int(np.count_nonzero(_size_mask(gt_areas_all, i, edges))) for i in range(len(_SIZE_KEYS))] for name, edges in schemes.items()}
        ap_overall = np.full(iou_thresholds.size, np.nan)
        recall_overall = np.full(iou_thresholds.size, np.nan)
        ap_size = {name: [np.full(iou_thresholds.size, np.nan) for _ in _SIZE_KEYS] for name in schemes}
        for ti, thr in enumerate(iou_thresholds):
            scores, matched, matched_gt_area, pred_area = self._match_masks_coco(float(thr))
            ap_overall[ti], recall_overall[ti] = _ap_from_pr(scores, matched, npig, recall_thresholds)
            for name, edges in schemes.items():
                for i in range(len(_SIZE_KEYS)):  # areaRng: TPs whose ground truth is in the bucket, FPs whose own area is; the rest is ignored
                    keep_tp = matched & _size_mask(matched_gt_area, i, edges)
                    keep = keep_tp | ((~matched) & _size_mask(pred_area, i, edges))
                    ap_size[name][i][ti], _ = _ap_from_pr(scores[keep], keep_tp[keep], n_gt_size[name][i], recall_thresholds)
        nanmean = lambda a: float(np.nanmean(a)) if np.any(~np.isnan(a)) else np.nan
        at = lambda t: float(ap_overall[int(np.argmin(np.abs(iou_thresholds - t)))])
        r = {"mask_voc.iou_thresholds": iou_thresholds, "mask_voc.AP": ap_overall, "mask_voc.recalls": recall_overall, "mask_voc.mAP": nanmean(ap_overall),
             "mask_voc.AR": nanmean(recall_overall), "mask_voc.AP50": at(0.5), "mask_voc.AP75": at(0.75), "mask_voc.n_gt": npig, "mask_voc.size_scheme": "percentile",
             "mask_voc.size_edges": [float(e) for e in schemes["percentile"]], "mask_voc.coco.size_edges": [float(e) for e in schemes["coco"]]}
        for name, prefix in (("percentile", "mask_voc."), ("coco", "mask_voc.coco.")):
            for i, bucket in enumerate(_SIZE_KEYS):
                r[f"{prefix}AP_{bucket}"] = nanmean(ap_size[name][i])
                r[f"{prefix}n_gt_{bucket}"] = n_gt_size[name][i]
        return r

    def evaluate(self) -> Dict[str, object]:
        return {"mask_metrics": self.mask_metrics(), "mask_voc_metrics": self.mask_voc_metrics()}


class SemanticEvaluator:
    """Whole-frame foreground metrics (``match_method="semantic"``): per frame the IoU and the boundary IoU of the predicted and the ground-truth
    foreground; frames whose ground-truth foreground is empty are skipped (``_process_frames_semantic``)."""

    def __init__(self) -> None:
        self.reset()

    def reset(self) -> None:
        self._rows: List[Tuple[float, float, float]] = []

    def __len__(self) -> int:
        return len(self._rows)

    def add_batch(self, pred_fg, gt_fg, pred_stride: int = 1) -> None:
        """``pred_fg (B, h, w)`` read at ``pred_stride``, ``gt_fg (B, H, W)``; nonzero = foreground."""
        s = int(pred_stride)
        stats = mask_pair_stats(pred_fg[:, None], gt_fg[:, None], pred_stride=s)
        keep = [b for b, (_, _, _, ga) in enumerate(stats) if ga[0] > 0]
        if not keep:
            return
        if _on_device(gt_fg):
            import torch

            idx = torch.as_tensor(keep, dtype=torch.long, device=gt_fg.device)
        else:
            pred_fg, gt_fg, idx = _to_numpy(pred_fg), _to_numpy(gt_fg), np.asarray(keep, dtype=np.int64)
        bious = boundary_iou(_upsample(pred_fg[idx] != 0, s), gt_fg[idx] != 0)
        self._rows.extend((float(stats[b][0][0, 0]), float("nan"), float(bi)) for b, bi in zip(keep, bious))

    def semantic_metrics(self) -> Dict[str, object]:
        rows = np.asarray(self._rows, dtype=float).reshape(-1, 3)
        ious, cldices, bious = rows[:, 0], rows[:, 1], rows[:, 2]
        cld_valid = cldices[~np.isnan(cldices)]
        return {"mean_iou": float(np.mean(ious)) if ious.size else float("nan"), "mean_cldice": float(np.mean(cld_valid)) if cld_valid.size else float("nan"),
                "mean_boundary_iou": float(np.mean(bious)) if bious.size else float("nan"), "ious": ious, "cldices": cldices, "boundary_ious": bious,
                "n_frames": int(ious.size)}


class EpochEndMaskEvaluator:
    """``EpochEndEvaluator`` for the segmentation model types: ``add_batch`` per validation batch (the arguments of ``MaskEvaluator.add_batch``, or
    ``(pred_fg, gt_fg[, pred_stride])`` with ``semantic=True``), ``compute(epoch)`` at the end of the epoch: the metrics dictionary on every
    ``eval_frequency``-th epoch, ``None`` otherwise (and when nothing was added); either way the collected frames are dropped."""

    def __init__(self, eval_frequency: int = 1, match_threshold: float = 0.5, semantic: bool = False) -> None:
        self.eval_frequency, self.semantic = int(eval_frequency), bool(semantic)
        self._ev = SemanticEvaluator() if semantic else MaskEvaluator(match_threshold)

    def due(self, epoch: int) -> bool:
        """Whether ``compute(epoch)`` will evaluate: a caller may skip ``add_batch`` in the other epochs."""
        return (epoch + 1) % self.eval_frequency == 0

    def add_batch(self, *args, **kwargs) -> None:
        self._ev.add_batch(*args, **kwargs)

    def compute(self, epoch: int = 0) -> Optional[Dict[str, object]]:
        out = None
        if self.due(epoch) and len(self._ev):
            out = {"semantic_metrics": self._ev.semantic_metrics()} if self.semantic else self._ev.evaluate()
        self._ev.reset()
        return out
