"""Fragment merge of bottom-up instance segmentation (``merge_instances``, sleap_nn/inference/segmentation.py:424-782): a region-adjacency graph over
a frame's candidate masks, agglomerated.  It runs after the argmin assignment and the distance gate, before the area floor and the packaging.

Two halves:

* the per-pixel part, ONE contract with two implementations -- ``ph_seg_merge_tables`` (csrc/seg_merge_kernels.hip) on the device label map, enqueued by
  ``group_enqueue`` and read with the grouping's one host read, and ``merge_tables_host`` in NumPy for CPU tensors (and as the comparison of the device
  in the tests).  Per frame with ``n`` centres and ``d = max(1, merge_dilate)``:

  - contact counts ``T[a][b]`` (a != b): the pixels labelled b with at least one pixel labelled a within L1 distance <= d inside the image (SciPy's
    default cross iterated d times, border value 0).  A pixel counts once per a; the reference's ``overlap(i, j)`` is ``T[i][j] + T[j][i]``;
  - moments per instance: sums over its pixels of ``rx, ry, rx^2, ry^2`` in float64, ``rx = (x - xc) s + dx`` -- the offset-predicted centre
    ``px = x s + s/2 + dx`` relative to the instance's own centre ``xc s + s/2``, so that the one-pass variance does not cancel;
  - the edge list: the pairs ``i < j`` with ``T[i][j] + T[j][i] > 0`` in (i, j) order as ``(i, j, T[i][j], T[j][i], ridge minimum)``; the ridge minimum
    is the float32 minimum of the centre map over the cells ``round(c_i + (c_j - c_i) k / 47)``, ``k = 7..39`` (``_center_valley_ridge`` with 48 samples).
    No sample is a rounding tie (a tie needs ``2 k delta = 47 (2 m + 1)``: even against odd), so the cells are computed in integers.

* the graph part on the host (tens of nodes): ``edge_affinities`` in float64 as the reference computes them, and ``agglomerate`` with the reference's
  two methods; ``merge_grouping`` applies the result to a ``Grouping`` (labels relabelled through a look-up table: label k is the k-th group).

Not built: ``merge_fragments`` together with ``mask_cleanup`` (cleaned masks overlap through their filled holes: the label map no longer carries membership).
"""
from __future__ import annotations

import math
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

DEFAULT_EDGE_CAP = 1024  # touching pairs per frame that the device's edge list holds
MAX_DILATE = 4  # diamonds the contact kernel is built for
MAX_MERGE_CENTERS = 4096  # the device's contact table is dense: max_centers^2 counters per frame
CONTACT_FLOOR = 1e-3
RIDGE_K = np.arange(7, 40, dtype=np.int64)  # the interior samples int(0.15 * 48) .. int(0.85 * 48) - 1 of 48
MERGE_DEFAULTS = dict(merge_method="greedy", merge_thresholds=(0.85, 0.6, 0.4), merge_w_valley=1.0, merge_w_offset=0.25, merge_dilate=1, join_bias=0.5)


def _check_method(method: str) -> None:
    if method not in ("greedy", "multicut", "none"):
        raise ValueError(f"unknown merge method {method!r} (merge_method is 'greedy', 'multicut' or 'none')")


def check_merge_args(merge_method: str, merge_dilate: int, device: bool, max_centers: Optional[int] = None) -> int:
    """Validate the knobs; returns ``d = max(1, merge_dilate)``.  The device kernel is built for ``d <= 4`` and at most 4096 centres."""
    _check_method(merge_method)
    d = max(1, int(merge_dilate))
    if device and d > MAX_DILATE:
        raise ValueError(f"merge_dilate={merge_dilate} is beyond the device kernel's diamond (merge_dilate <= {MAX_DILATE})")
    if device and max_centers is not None and int(max_centers) > MAX_MERGE_CENTERS:
        raise ValueError(f"merge_fragments holds at most max_centers={MAX_MERGE_CENTERS} centres per frame on the device (a dense contact table), got {max_centers}")
    return d


# ---- the per-pixel part on the host ---------------------------------------------------------------------------------------------

def _dilate_diamond(m: np.ndarray, d: int) -> np.ndarray:
    out = m.copy()
    for _ in range(d):
        g = out.copy()
        g[1:] |= out[:-1]
        g[:-1] |= out[1:]
        g[:, 1:] |= out[:, :-1]
        g[:, :-1] |= out[:, 1:]
        out = g
    return out


def ridge_minimum(hm: np.ndarray, ca, cb) -> np.float32:
    """Float32 minimum of ``hm`` (h, w) over the 33 interior samples of the line between the integer grid centres ``ca`` and ``cb`` = (x, y)."""
    h, w = hm.shape
    xi = np.clip((2 * (47 * int(ca[0]) + (int(cb[0]) - int(ca[0])) * RIDGE_K) + 47) // 94, 0, w - 1)
    yi = np.clip((2 * (47 * int(ca[1]) + (int(cb[1]) - int(ca[1])) * RIDGE_K) + 47) // 94, 0, h - 1)
    return np.float32(hm[yi, xi].min())


def merge_tables_host(labels, hm, off, centers, n: int, output_stride: int, dilate: int):
    """One frame: ``labels`` (h, w) integers (-1 = background), ``hm`` (h, w) and ``off`` (2, h, w) float32, ``centers`` (>= n, 2) integer (x, y) ->
    ``(T (n, n) int64, moments (n, 4) float64, edges (E, 4) int64 = (i, j, T[i][j], T[j][i]), ridge (E,) float32)``: the contract of ``ph_seg_merge_tables``."""
    lab = np.asarray(labels).astype(np.int64)
    hm = np.asarray(hm, dtype=np.float32)
    off = np.asarray(off, dtype=np.float32)
    n = int(n)
    d = max(1, int(dilate))
    s = int(output_stride)
    lab = np.where((lab >= 0) & (lab < n), lab, -1)
    T = np.zeros((n, n), dtype=np.int64)
    mom = np.zeros((n, 4), dtype=np.float64)
    for a in range(n):
        m = lab == a
        if not m.any():
            continue
        near = _dilate_diamond(m, d) & (lab >= 0) & ~m
        T[a] = np.bincount(lab[near], minlength=n)
        ys, xs = np.nonzero(m)
        rx = ((xs - int(centers[a][0])) * s).astype(np.float64) + off[0][ys, xs].astype(np.float64)
        ry = ((ys - int(centers[a][1])) * s).astype(np.float64) + off[1][ys, xs].astype(np.float64)
        mom[a] = (rx.sum(), ry.sum(), (rx * rx).sum(), (ry * ry).sum())
    both = T + T.T
    ii, jj = np.nonzero(np.triu(both, 1) > 0)  # row-major: (i, j) order
    edges = np.stack([ii, jj, T[ii, jj], T[jj, ii]], axis=1).astype(np.int64).reshape(-1, 4)
    ridge = np.array([ridge_minimum(hm, centers[i], centers[j]) for i, j in zip(ii, jj)], dtype=np.float32)
    return T, mom, edges, ridge


# ---- the graph part -------------------------------------------------------------------------------------------------------------------

def edge_affinities(edges, ridge, moments, areas, centers, scores, output_stride: int, w_valley: float = 1.0, w_offset: float = 0.25,
                    detail: Optional[list] = None) -> List[Tuple[int, int, float]]:
    """``_build_merge_rag`` from the tables: ``[(i, j, affinity)]`` in edge-list order, in float64 as the reference computes them.

    ``contact = overlap / max(1, min(area_i, area_j))``, dropped at ``contact <= 1e-3``; ``contact_gate = min(1, contact / 0.05)``; with
    ``w_valley + w_offset <= 0`` the affinity is the gate.  Otherwise ``ridge = clip(min / max(1e-6, min(score_i, score_j)), 0, 1)`` -- a float32 quotient,
    as NumPy (>= 2) evaluates the reference's float32-by-Python-float division -- and ``offset = exp(-sep^2 / (2 (2 scale)^2))``, ``scale = max(spread, stride)``:
    ``sep`` the distance of the two mean offset-predicted centres, ``spread`` the mean of the four population standard deviations.  ``detail`` (a list)
    receives ``(i, j, overlap, contact, ridge, offset)`` per kept edge."""
    s = float(output_stride)
    wsum = w_valley + w_offset
    areas = np.asarray(areas, dtype=np.int64)

    def cloud(k):
        nk = float(areas[k])
        mx, my = moments[k][0] / nk, moments[k][1] / nk
        sdx = math.sqrt(max(0.0, moments[k][2] / nk - mx * mx))
        sdy = math.sqrt(max(0.0, moments[k][3] / nk - my * my))
        return float(centers[k][0]) * s + s / 2.0 + mx, float(centers[k][1]) * s + s / 2.0 + my, 0.5 * (sdx + sdy)

    out = []
    for (i, j, tij, tji), rmin in zip(np.asarray(edges).reshape(-1, 4).tolist(), np.asarray(ridge, dtype=np.float32).reshape(-1)):
        overlap = int(tij) + int(tji)
        if overlap == 0:
            continue
        contact = overlap / max(1, min(int(areas[i]), int(areas[j])))
        if contact <= CONTACT_FLOOR:
            continue
        gate = min(1.0, contact / 0.05)
        if wsum <= 0:
            out.append((i, j, gate))
            if detail is not None:
                detail.append((i, j, overlap, contact, None, None))
            continue
        denom = max(1e-6, min(float(scores[i]), float(scores[j])))
        rid = float(np.clip(np.float32(rmin) / np.float32(denom), 0.0, 1.0))
        ax, ay, asd = cloud(i)
        bx, by, bsd = cloud(j)
        sep = math.hypot(ax - bx, ay - by)
        scale = max(0.5 * (asd + bsd), s)
        agree = math.exp(-(sep**2) / (2.0 * (2.0 * scale) ** 2))
        out.append((i, j, float(gate * ((w_valley * rid + w_offset * agree) / wsum))))
        if detail is not None:
            detail.append((i, j, overlap, contact, rid, agree))
    return out


def agglomerate(n: int, affinities: Sequence[Tuple[int, int, float]], method: str = "greedy", thresholds: Sequence[float] = (0.85, 0.6, 0.4),
                join_bias: float = 0.5, trace: Optional[list] = None) -> List[List[int]]:
    """Partition of the nodes ``0..n-1``: sorted member lists, ordered by their smallest member.

    ``"greedy"``: one phase per threshold; while the live edge with the largest mean member affinity (the first in edge order on ties) is ``>=`` the
    threshold it is contracted; parallel edges concatenate their member lists.  ``"multicut"``: ``cost = logit(clamp(aff, 1e-4, 1 - 1e-4)) - logit(join_bias)``;
    the largest cost is contracted while it is ``> 0``; parallel costs add.  Edge order after a contraction: first appearance while walking the previous
    order.  ``trace`` (a list) receives one ``(value, runner_up or None, compared_with, contracted)`` per decision -- every contraction and every stop."""
    _check_method(method)
    root = list(range(n))
    if method != "none" and n > 1:
        if method == "greedy":
            live: Dict[Tuple[int, int], list] = {}
            for i, j, a in affinities:
                live.setdefault((min(i, j), max(i, j)), []).append(float(a))
            # np.mean as the reference takes it; below eight members NumPy adds left to right, which plain Python does as well and much faster
            value = lambda v: sum(v) / len(v) if len(v) < 8 else float(np.mean(v))
            join = lambda old, new: old + new
            phases = [(float(t), True) for t in thresholds]
        else:
            logit = lambda p: math.log(min(max(p, 1e-4), 1 - 1e-4) / (1 - min(max(p, 1e-4), 1 - 1e-4)))
            live = {}
            for i, j, a in affinities:
                k = (min(i, j), max(i, j))
                c = logit(float(a)) - logit(join_bias)
                live[k] = live[k] + c if k in live else c
            value = lambda v: v
            join = lambda old, new: old + new
            phases = [(0.0, False)]
        for bound, inclusive in phases:
            while True:
                best, best_v, second = None, (-1.0 if inclusive else -math.inf), None
                for key, v in live.items():
                    x = value(v)
                    if x > best_v:
                        if best is not None:
                            second = best_v
                        best, best_v = key, x
                    elif second is None or x > second:
                        second = x
                go = best is not None and (best_v >= bound if inclusive else best_v > bound)
                if trace is not None and best is not None:
                    trace.append((best_v, second, bound, go))
                if not go:
                    break
                keep, gone = best
                root = [keep if r == gone else r for r in root]
                merged: Dict[Tuple[int, int], object] = {}
                for (a, b), v in live.items():
                    a, b = (keep if a == gone else a), (keep if b == gone else b)
                    if a == b:
                        continue
                    k = (min(a, b), max(a, b))
                    merged[k] = join(merged[k], v) if k in merged else (list(v) if isinstance(v, list) else v)
                live = merged
    groups: Dict[int, List[int]] = {}
    for k in range(n):
        groups.setdefault(root[k], []).append(k)
    return list(groups.values())


def merge_frame(labels: np.ndarray, centers: np.ndarray, scores: np.ndarray, counts: np.ndarray, edges, ridge, moments, output_stride: int,
                method: str = "greedy", thresholds: Sequence[float] = (0.85, 0.6, 0.4), w_valley: float = 1.0, w_offset: float = 0.25, join_bias: float = 0.5,
                trace: Optional[dict] = None):
    """One frame of a ``Grouping`` after the merge: ``(labels, centers, scores, counts, members)``.  Every centre is a node (one without pixels has no edge and
    stays a group of its own, dropped later like today); a group's representative is its highest-scoring member (the first on ties), its count the sum.
    ``method="none"`` or fewer than two instances with pixels change nothing.  ``trace`` (a dict) receives ``"edges"``, ``"detail"`` and ``"decisions"``."""
    n = len(centers)
    counts = np.asarray(counts)
    _check_method(method)
    if method == "none" or int((counts > 0).sum()) < 2:
        return labels, centers, scores, counts, [[k] for k in range(n)]
    detail = [] if trace is not None else None
    decisions = [] if trace is not None else None
    aff = edge_affinities(edges, ridge, moments, counts, centers, scores, output_stride, w_valley, w_offset, detail=detail)
    groups = agglomerate(n, aff, method, thresholds, join_bias, trace=decisions)
    if trace is not None:
        trace.update(edges=aff, detail=detail, decisions=decisions)
    if len(groups) == n:  # nothing was contracted: every centre is its own group, in order
        return labels, centers, scores, counts, groups
    lut = np.full(n + 1, -1, dtype=labels.dtype)  # (the last entry serves the label -1)
    rep = []
    for g, members in enumerate(groups):
        lut[members] = g
        rep.append(max(members, key=lambda k: scores[k]))  # (max keeps the first of equal scores)
    return (lut.take(labels, mode="wrap"), centers[rep], scores[rep], np.array([int(counts[m].sum()) for m in groups], dtype=counts.dtype), groups)
