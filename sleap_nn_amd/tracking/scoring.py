"""Features and pair scores of the tracker (sleap_nn/tracking/utils.py:47-252, ``compute_oks`` of sleap_nn/evaluation.py:644-760 as the tracker calls it).

Every score is a function of ONE (current instance, past instance) pair, so a batch's scores can be computed before the sequential part of the tracker runs:

* NumPy, pair by pair (this module's ``oks_score`` / ``bbox_iou`` / ``neg_euclidean`` / ``cosine_sim`` / ``mask_iou``): the reference's arithmetic restated.  It is what
  ``Tracker.track`` uses, what a ``local_queues`` candidate older than the table's reach falls back to, and what the CPU tests compare the native call against;
* ``pose_pair_scores``: ``ph_track_pose_scores`` (csrc/track_host.cpp), all pairs of a batch against the batch itself and the history in one native call;
* ``mask_pair_counts``: ``ph_track_mask_pairs`` (csrc/track_kernels.hip), the weighted contingency tables of a batch of device label maps against the batch
  itself and the device ring of earlier label maps; ``mask_iou_table`` turns them into IoUs in float64 on the host.

Mask IoU lives on the IMAGE grid (``decode_mask_to_image_res``: nearest resample of the stride-resolution mask to its image extent).  That resample is separable
and uses the integer rule ``(u * w) // We`` (``place_crop_masks``), so a cell (v, u) of the label map stands for ``rows(v) * cols(u)`` image pixels;
``axis_weights`` builds both vectors with ``np.bincount`` of the per-axis index maps, and the weighted counts are exactly the image-grid intersections and areas.
"""
from __future__ import annotations

import ctypes as C
import warnings
from typing import Optional, Tuple

import numpy as np

METHODS = {"oks": 0, "iou": 1, "euclidean_dist": 2, "cosine_sim": 3}
MAX_TABLE_LAGS = 32  # ph_track_pose_scores / ph_track_mask_pairs: lags per call
MAX_TABLE_LABELS = 64  # ph_track_mask_pairs: labels per frame


# ---- features (utils.py:47-76) --------------------------------------------------------------------------------------

def keypoints_feature(points: np.ndarray) -> np.ndarray:
    return points


def centroid_feature(points: np.ndarray) -> np.ndarray:
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", category=RuntimeWarning)
        return np.nanmedian(points, axis=0)


def bbox_feature(points: np.ndarray) -> np.ndarray:
    """``[xmin, ymin, xmax, ymax]``."""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", category=RuntimeWarning)
        return np.concatenate([np.nanmin(points, axis=0), np.nanmax(points, axis=0)])


def count_valid_points(points: np.ndarray) -> int:
    return int((~np.isnan(points).any(axis=1)).sum())


# ---- pose scores, one pair ------------------------------------------------------------------------------------------

def oks_score(points_gt: np.ndarray, points_pr: np.ndarray, stddev: float = 0.025) -> float:
    """``compute_oks(points_gt, points_pr, stddev=stddev)`` for one pair: the current instance is ``points_gt``, its bounding-box area the scale."""
    gt = np.asarray(points_gt, dtype=np.float64)
    pr = np.asarray(points_pr, dtype=np.float64)
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore", category=RuntimeWarning)
        scale = np.prod(np.nanmax(gt, axis=0) - np.nanmin(gt, axis=0))
        distance = ((gt - pr) ** 2).sum(axis=-1)
        norm = ((2 * stddev) ** 2) * (2 * (scale + np.spacing(1)))
        distance[np.any(np.isnan(pr), axis=-1)] = np.inf
        ks = np.exp(-(distance / norm))
        missing_gt = np.any(np.isnan(gt), axis=-1)
        ks[missing_gt] = 0
        n_visible = np.sum((~missing_gt).astype("float32"))
        return float(np.sum(ks) / n_visible)


def bbox_iou(a, b) -> float:
    """``compute_iou`` with its ``+ 1``s; Python's ``max`` / ``min`` (the first argument wins when a comparison with NaN is false)."""
    (xmin1, ymin1, xmax1, ymax1), (xmin2, ymin2, xmax2, ymax2) = (float(v) for v in a), (float(v) for v in b)
    ix = max(0, min(xmax1, xmax2) - max(xmin1, xmin2) + 1)
    iy = max(0, min(ymax1, ymax2) - max(ymin1, ymin2) + 1)
    inter = ix * iy
    union = (xmax1 - xmin1 + 1) * (ymax1 - ymin1 + 1) + (xmax2 - xmin2 + 1) * (ymax2 - ymin2 + 1) - inter
    with np.errstate(all="ignore"):
        return float(np.float64(inter) / np.float64(union))


def neg_euclidean(a, b) -> float:
    return float(-np.linalg.norm(np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)))


def cosine_sim(a, b) -> float:
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    with np.errstate(all="ignore"):
        return float(np.dot(a, b) / (np.linalg.norm(a) * np.linalg.norm(b)))


# ---- masks ----------------------------------------------------------------------------------------------------------

class MaskFeature:
    """A mask on the image grid as its tight bounding-box crop, the crop's top-left ``(y0, x0)`` and the foreground area in image pixels."""

    __slots__ = ("crop", "y0", "x0", "area")

    def __init__(self, crop: np.ndarray, y0: int, x0: int, area: int):
        self.crop, self.y0, self.x0, self.area = crop, int(y0), int(x0), int(area)


def decode_to_image(entry: dict) -> np.ndarray:
    """A ``pred_masks`` entry on the image grid (``decode_mask_to_image_res``): nearest resample to ``(round(h / sy), round(w / sx))`` by the integer rule,
    then the rounded offset as a top-left pad, negative rows / columns dropped."""
    m = np.asarray(entry["mask"], dtype=bool)
    scale = tuple(float(s) for s in entry.get("scale", (1.0, 1.0)))
    offset = tuple(float(o) for o in entry.get("offset", (0.0, 0.0)))
    if scale != (1.0, 1.0):
        h, w = m.shape
        He, We = int(round(h / scale[1])), int(round(w / scale[0]))
        rows, cols = (np.arange(He, dtype=np.int64) * h) // max(He, 1), (np.arange(We, dtype=np.int64) * w) // max(We, 1)
        m = m[rows[:, None], cols[None, :]]
    ox, oy = int(round(offset[0])), int(round(offset[1]))
    if ox or oy:
        src = m[max(0, -oy):, max(0, -ox):]
        out = np.zeros((max(0, oy) + src.shape[0], max(0, ox) + src.shape[1]), dtype=bool)
        out[max(0, oy):, max(0, ox):] = src
        m = out
    return m


def mask_feature(entry) -> MaskFeature:
    """The ``"masks"`` feature of a ``pred_masks`` entry (or of a dense bool array already on the image grid)."""
    if isinstance(entry, MaskFeature):
        return entry
    data = decode_to_image(entry) if isinstance(entry, dict) else np.asarray(entry, dtype=bool)
    rows = np.any(data, axis=1)
    if not rows.any():
        return MaskFeature(np.zeros((0, 0), dtype=bool), 0, 0, 0)
    cols = np.any(data, axis=0)
    y0, y1 = int(np.argmax(rows)), len(rows) - int(np.argmax(rows[::-1]))
    x0, x1 = int(np.argmax(cols)), len(cols) - int(np.argmax(cols[::-1]))
    crop = data[y0:y1, x0:x1]
    return MaskFeature(crop, y0, x0, int(np.count_nonzero(crop)))


def mask_intersection(fa: MaskFeature, fb: MaskFeature) -> int:
    if fa.area == 0 or fb.area == 0:
        return 0
    oy0, oy1 = max(fa.y0, fb.y0), min(fa.y0 + fa.crop.shape[0], fb.y0 + fb.crop.shape[0])
    ox0, ox1 = max(fa.x0, fb.x0), min(fa.x0 + fa.crop.shape[1], fb.x0 + fb.crop.shape[1])
    if oy1 <= oy0 or ox1 <= ox0:
        return 0
    return int(np.count_nonzero(fa.crop[oy0 - fa.y0 : oy1 - fa.y0, ox0 - fa.x0 : ox1 - fa.x0] & fb.crop[oy0 - fb.y0 : oy1 - fb.y0, ox0 - fb.x0 : ox1 - fb.x0]))


def mask_iou(a, b) -> float:
    """Pixel IoU of two masks on the image grid; 1.0 for empty against empty."""
    fa, fb = mask_feature(a), mask_feature(b)
    inter = mask_intersection(fa, fb)
    union = fa.area + fb.area - inter
    return 1.0 if union == 0 else float(inter / union)


def axis_weights(row_index: np.ndarray, col_index: np.ndarray, h: int, w: int) -> Tuple[np.ndarray, np.ndarray]:
    """``row_index[Y]`` / ``col_index[X]``: the label-map row / column image row Y / column X reads (the layer's per-axis index maps).  Returns
    ``(row_weight int32 (h,), col_weight int32 (w,))``: the image rows / columns each cell row / column stands for; cells in the padding stand for none."""
    return np.bincount(np.asarray(row_index, dtype=np.int64), minlength=h).astype(np.int32), np.bincount(np.asarray(col_index, dtype=np.int64), minlength=w).astype(np.int32)


def mask_iou_table(inter: np.ndarray, area_cur: np.ndarray, area_past: np.ndarray) -> np.ndarray:
    """``inter (..., P, P)``, ``area_cur (..., P)``, ``area_past (..., P)`` integers -> IoU float64 ``inter / (a + b - inter)``, 1.0 where the union is 0."""
    inter = inter.astype(np.int64)
    union = area_cur.astype(np.int64)[..., :, None] + area_past.astype(np.int64)[..., None, :] - inter
    out = np.ones(inter.shape, dtype=np.float64)
    np.divide(inter, union, out=out, where=union != 0)
    return out


# ---- native tables --------------------------------------------------------------------------------------------------

def pose_pair_scores(cur: np.ndarray, hist: Optional[np.ndarray], n_hist: int, counts: np.ndarray, method: str, oks_stddev: float = 0.025, lags: Optional[int] = None) -> np.ndarray:
    """``ph_track_pose_scores``: ``cur`` float64 (B, I, N, 2) features of the batch's frames, ``hist`` (L, I, N, 2) those of earlier frames, newest last, the
    last ``n_hist`` valid; ``counts`` int32 (B + L,): instances of each ``cur`` frame, then of each ``hist`` slot.  Returns float64 (B, L, I, I):
    ``[b][k - 1][i][j]`` = the score of instance i of frame b against instance j of the frame k calls earlier (``cur[b - k]`` if ``b >= k``, else
    ``hist[L - (k - b)]``); NaN where either instance is beyond its frame's count or the lag reaches beyond ``n_hist``."""
    from sleap_nn_amd import _lib as L_

    cur = np.ascontiguousarray(cur, dtype=np.float64)
    B, I, N = cur.shape[0], cur.shape[1], cur.shape[2]
    if hist is None:
        lags = int(lags if lags is not None else 1)
        hist = np.zeros((lags, I, N, 2), dtype=np.float64)
        n_hist = 0
    hist = np.ascontiguousarray(hist, dtype=np.float64)
    L = hist.shape[0]
    if hist.shape[1:] != cur.shape[1:]:
        raise ValueError(f"pose_pair_scores: cur {cur.shape} and hist {hist.shape} differ beyond their first axis")
    counts = np.ascontiguousarray(counts, dtype=np.int32)
    if counts.shape != (B + L,):
        raise ValueError(f"pose_pair_scores: counts has shape {counts.shape}, expected ({B + L},)")
    if method not in METHODS:
        raise ValueError(f"pose_pair_scores: method must be one of {sorted(METHODS)}, got {method!r}")
    out = np.empty((B, L, I, I), dtype=np.float64)
    p = lambda a: C.c_void_p(a.ctypes.data)
    L_.check(L_.lib().ph_track_pose_scores(p(cur), B, p(hist), L, int(n_hist), I, N, p(counts), METHODS[method], float(oks_stddev), p(out)))
    return out


def mask_pair_counts(labels, hist, n_hist: int, row_weight, col_weight, P: int, image_pixels: int):
    """``ph_track_mask_pairs`` on the current stream: ``labels`` (B, h, w) and ``hist`` (L, h, w) signed-integer device tensors of one dtype (-1 = background,
    labels at or beyond ``P`` count as background; ``hist`` newest last, the last ``n_hist`` valid), ``row_weight`` int32 (h,) / ``col_weight`` int32 (w,) device
    tensors.  Returns ONE int32 device tensor ``[inter (B, L, P, P) | area (B, P)]`` (a single device-to-host copy reads both) and the two views.  No host
    synchronisation."""
    import torch

    from sleap_nn_amd import _lib as L_

    L_.require_cuda(labels, "labels")
    labels, hist = labels.contiguous(), hist.contiguous()
    if labels.dtype != hist.dtype or labels.dtype not in (torch.int8, torch.int16, torch.int32):
        raise ValueError(f"mask_pair_counts: labels {labels.dtype} and hist {hist.dtype} must share one of int8 / int16 / int32")
    B, h, w = labels.shape
    L = int(hist.shape[0])
    if tuple(hist.shape[1:]) != (h, w):
        raise ValueError(f"mask_pair_counts: hist {tuple(hist.shape)} does not match the {h} x {w} maps")
    rw = row_weight.to(labels.device, torch.int32).contiguous()
    cw = col_weight.to(labels.device, torch.int32).contiguous()
    if rw.numel() != h or cw.numel() != w:
        raise ValueError(f"mask_pair_counts: {rw.numel()} row and {cw.numel()} column weights for {h} x {w} maps")
    P = int(P)
    with torch.cuda.device(labels.device):
        rec = torch.empty(B * L * P * P + B * P, dtype=torch.int32, device=labels.device)
        inter, area = rec[: B * L * P * P].view(B, L, P, P), rec[B * L * P * P :].view(B, P)
        p = lambda t: C.c_void_p(t.data_ptr())
        L_.check(L_.lib().ph_track_mask_pairs(p(labels), labels.element_size(), B, h, w, p(hist), L, int(n_hist), p(rw), p(cw), int(image_pixels), P, p(inter), p(area),
                                              L_.current_stream_ptr()))
    return rec, inter, area


def pose_pair_scores_shifted(cur: np.ndarray, hist: np.ndarray, counts_cur: np.ndarray, counts_hist: np.ndarray, method: str, oks_stddev: float = 0.025) -> np.ndarray:
    """``ph_track_pose_scores_shifted``: ``cur`` float64 (B, I, N, 2) features of the batch's frames; ``hist`` (B, L, I, N, 2): per current frame b and group g (a
    lag, or a reference frame) the features of that group's candidates AS SEEN FROM frame b (the flow-shift tracker moves a past instance onto each current frame);
    ``counts_cur`` int32 (B,), ``counts_hist`` int32 (B, L).  Returns float64 (B, L, I, I): ``[b][g][i][j]`` = the score of instance i of frame b against candidate
    j of group g, NaN beyond a count."""
    from sleap_nn_amd import _lib as L_

    cur = np.ascontiguousarray(cur, dtype=np.float64)
    hist = np.ascontiguousarray(hist, dtype=np.float64)
    B, I, N = cur.shape[0], cur.shape[1], cur.shape[2]
    if hist.ndim != 5 or hist.shape[0] != B or hist.shape[2:] != cur.shape[1:]:
        raise ValueError(f"pose_pair_scores_shifted: cur {cur.shape} and hist {hist.shape} do not fit (B, I, N, 2) / (B, L, I, N, 2)")
    L = hist.shape[1]
    counts_cur = np.ascontiguousarray(counts_cur, dtype=np.int32)
    counts_hist = np.ascontiguousarray(counts_hist, dtype=np.int32)
    if counts_cur.shape != (B,) or counts_hist.shape != (B, L):
        raise ValueError(f"pose_pair_scores_shifted: counts of shapes {counts_cur.shape} / {counts_hist.shape}, expected ({B},) / ({B}, {L})")
    if method not in METHODS:
        raise ValueError(f"pose_pair_scores_shifted: method must be one of {sorted(METHODS)}, got {method!r}")
    out = np.empty((B, L, I, I), dtype=np.float64)
    p = lambda a: C.c_void_p(a.ctypes.data)
    L_.check(L_.lib().ph_track_pose_scores_shifted(p(cur), B, p(hist), L, I, N, p(counts_cur), p(counts_hist), METHODS[method], float(oks_stddev), p(out)))
    return out
