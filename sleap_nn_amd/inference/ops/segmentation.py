"""Grouping of foreground pixels into instances (sleap_nn/inference/segmentation.py:12-237) as a label map.

Two implementations of ONE contract, ``group_instances_from_offsets(...) -> Grouping``:

* the device path (``ph_seg_center_peaks`` + ``ph_seg_assign`` + ``ph_seg_gate``, csrc/seg_kernels.hip): a fixed sequence of launches on the current stream,
  then one host read per batch -- the label map in the narrowest integer type that holds the centre count, and one small pinned
  record with the centres, scores and pixel counts;
* a plain torch / numpy host implementation, used for CPU tensors and pinned against the reference's recorded results by the CPU tests.

The contract (what the reference computes, frame by frame):

* centre candidates: ``hm >= max over the k x k window (-inf outside)`` and ``hm > peak_threshold``; candidates that touch by 4-connectivity are one
  component, represented by its maximum value (raster-first on ties); components are numbered by their raster-first pixel.  With ``max_instances`` set
  and more components, the ``max_instances`` largest values in descending order;
* every pixel with ``fg > fg_threshold`` gets the first argmin over centres of ``(px - cx)^2 + (py - cy)^2`` in fp32, ``px = x s + s/2 + dx``,
  ``cx = xc s + s/2`` (likewise y);
* the adaptive distance gate re-estimates ``r^2 = (alpha sqrt(count / pi) s)^2`` for ``distance_gate_iters`` passes from the currently kept pixels and
  keeps ``d <= r^2[label]``, recomputed over all assigned pixels each pass;
* a frame without foreground or without centres has no instances; instances left without pixels are dropped, the others keep their order;
* ``mask_cleanup=True`` (``_clean_instance_mask`` at radius 0, segmentation.py:240-273), per instance after assignment and gate: of its 4-connected
  components the one with the most pixels is kept (raster-first on ties), then every complement pixel that cannot reach the outside of the image by
  4-connected steps through the complement joins the mask (``binary_fill_holes``; other instances' pixels are complement, so masks may overlap).  The label
  map then holds the kept components and ``Grouping.holes`` the filled pixels; ``ph_seg_cleanup`` (csrc/seg_cleanup_kernels.hip) on the device,
  ``clean_label_map`` on the host;
* ``merge_fragments=True`` (``merge_instances``, segmentation.py:424-782), per frame after assignment and gate: a region-adjacency graph over the candidate
  masks (contact by dilation, centre-map ridge, offset agreement), agglomerated by ``"greedy"`` or ``"multicut"``.  The per-pixel tables come from
  ``ph_seg_merge_tables`` (csrc/seg_merge_kernels.hip) on the device label map with the same host read, or from ``merge_tables_host``; the graph is host work
  (``inference/ops/segmentation_merge.py``).  The label map is then relabelled: label k is the k-th group, ``Grouping.members`` names each group's centres.
  Not built: ``mask_cleanup_radius > 0`` (OpenCV's elliptical open / close) and ``merge_fragments`` together with ``mask_cleanup`` (cleaned masks overlap
  through their filled holes: the label map no longer carries membership).

Also here: the semantic threshold / count / sum (``semantic_masks``) and the geometry and placement of top-down crop masks
(``crop_mask_geometry``, ``place_crop_masks``: ``ph_seg_place_crops`` on the device, NumPy on the host, one contract).
"""
from __future__ import annotations

import ctypes as C
import math
import threading
from collections import OrderedDict
from dataclasses import dataclass
from typing import Dict, List, NamedTuple, Optional

import numpy as np
import torch
import torch.nn.functional as F

from sleap_nn_amd.inference.ops.segmentation_merge import DEFAULT_EDGE_CAP, MERGE_DEFAULTS, check_merge_args, merge_frame, merge_tables_host

DEFAULT_CAP = 2048  # candidates per frame that the collapse kernel keeps in LDS
DEFAULT_MAX_CENTERS = 127  # centres per frame that one-byte labels hold
DEFAULT_HOLE_CAP = 4096  # filled hole pixels per frame that the cleanup's list holds


@dataclass
class Grouping:
    """``labels`` (B, h, w) signed integers, -1 = background, otherwise an index into the frame's centres; per frame ``centers`` (N, 2) int32 (x, y) in map
    pixels, ``scores`` (N,) float32 (the centre's peak value) and ``counts`` (N,) the pixels each centre kept.  After mask cleanup ``labels`` holds each
    instance's kept component, ``holes`` per frame the filled pixels as int32 (K, 2) = (pixel index y * w + x, label), instance-major and in raster order
    inside an instance (they may lie on other instances' pixels), and ``counts`` the cleaned areas (component + holes).  After the fragment merge an entry
    is a group: ``labels`` index the groups, ``centers`` / ``scores`` are the representative's, ``counts`` the members' sum, and ``members`` per frame lists
    each group's original centre indices.  ``labels_dev``: on the device path without cleanup or merge, the device tensor ``labels`` was read from (the mask
    tracker's tables read it in place)."""

    labels: np.ndarray
    centers: List[np.ndarray]
    scores: List[np.ndarray]
    counts: List[np.ndarray]
    holes: Optional[List[np.ndarray]] = None
    members: Optional[List[List[List[int]]]] = None
    labels_dev: Optional[torch.Tensor] = None

    def instances(self, b: int, output_stride: int) -> List[Dict]:
        """The reference's per-frame list (segmentation.py:213-237): ``{"mask", "center", "score"}`` per non-empty instance, in centre order; ``center`` in input pixels."""
        out = []
        lab = self.labels[b]
        s = np.float32(output_stride)
        half = np.float32(output_stride / 2.0)
        holes = self.holes[b] if self.holes is not None else None
        for k in np.nonzero(self.counts[b] > 0)[0]:
            cx, cy = self.centers[b][k]
            mask = lab == k
            if holes is not None and len(holes):
                mask.reshape(-1)[holes[holes[:, 1] == k, 0]] = True
            out.append({"mask": mask, "center": (float(np.float32(cx) * s + half), float(np.float32(cy) * s + half)), "score": float(self.scores[b][k])})
        return out


def label_dtype(max_centers: int):
    return torch.int8 if max_centers <= 127 else (torch.int16 if max_centers <= 32767 else torch.int32)


# ---- host implementation ------------------------------------------------------------------------------------------

def find_center_peaks_host(hm: torch.Tensor, threshold: float, kernel_size: int = 3):
    """``hm`` (h, w) float32 on the CPU -> (centres (N, 2) int32 (x, y), values (N,) float32)."""
    k = int(kernel_size)
    pooled = F.max_pool2d(hm[None, None], kernel_size=k, stride=1, padding=k // 2)[0, 0]
    cand = ((hm >= pooled) & (hm > threshold)).numpy()
    ys, xs = np.nonzero(cand)  # raster order
    n = len(ys)
    if n == 0:
        return np.zeros((0, 2), np.int32), np.zeros((0,), np.float32)
    w = hm.shape[1]
    index = {int(y) * w + int(x): i for i, (y, x) in enumerate(zip(ys, xs))}
    parent = list(range(n))

    def find(i):
        while parent[i] != i:
            parent[i] = parent[parent[i]]
            i = parent[i]
        return i

    for i, (y, x) in enumerate(zip(ys, xs)):
        for j in ((index.get(int(y) * w + int(x) - 1) if x > 0 else None), index.get((int(y) - 1) * w + int(x)) if y > 0 else None):
            if j is not None:
                a, c = find(i), find(j)
                if a != c:
                    parent[max(a, c)] = min(a, c)  # the root is the raster-first member
    vals = hm.numpy()[ys, xs]
    best: Dict[int, int] = {}
    for i in range(n):  # ascending index: a later member replaces the representative only when strictly larger
        r = find(i)
        if r not in best or vals[i] > vals[best[r]]:
            best[r] = i
    reps = [best[r] for r in sorted(best)]
    return np.stack([xs[reps], ys[reps]], axis=1).astype(np.int32), vals[reps].astype(np.float32)


def _components(lab: np.ndarray) -> np.ndarray:
    """``lab`` (h, w) integers -> int64 (h, w): the raster-first pixel index of each pixel's component, -1 where ``lab < 0``.  Two 4-neighbours are joined
    when they carry the same non-negative value.  Union-find over the rows' runs of equal values; a root is always the earliest run of its tree."""
    h, w = lab.shape
    flat = lab.reshape(-1)
    start = np.ones(h * w, dtype=bool)
    start[1:] = flat[1:] != flat[:-1]
    start[::w] = True
    run_of = (np.cumsum(start) - 1).reshape(h, w)
    run_start = np.nonzero(start)[0]
    parent = list(range(len(run_start)))

    def find(i):
        while parent[i] != i:
            parent[i] = parent[parent[i]]
            i = parent[i]
        return i

    if h > 1:
        join = (lab[1:] == lab[:-1]) & (lab[1:] >= 0)
        pairs = np.unique(np.stack([run_of[1:][join], run_of[:-1][join]], axis=1), axis=0)
        for a, c in pairs.tolist():
            a, c = find(a), find(c)
            if a != c:
                parent[max(a, c)] = min(a, c)
    root = np.array([find(i) for i in range(len(parent))], dtype=np.int64)
    comp = run_start[root][run_of]
    comp[lab < 0] = -1
    return comp


def clean_label_map(labels: np.ndarray, n_centers: int):
    """Mask cleanup of one frame's label map (h, w) on the host: ``(cleaned (h, w), holes int32 (K, 2), areas int32 (n_centers,))`` -- the contract of
    ``ph_seg_cleanup``: per label the largest 4-connected component (raster-first on ties) stays in ``cleaned``, the others become -1; ``holes`` lists the
    pixels ``binary_fill_holes`` adds to each kept component as (pixel index, label), instance-major, raster order inside an instance; ``areas`` = component +
    holes.  The flood runs over the component's bounding box grown by a one-pixel ring: everything beyond is connected to the outside."""
    lab = np.asarray(labels)
    h, w = lab.shape
    n = int(n_centers)
    cleaned = np.full_like(lab, -1)
    areas = np.zeros(n, dtype=np.int32)
    holes: List[np.ndarray] = []
    comp = _components(np.where(lab < n, lab, -1))
    on = comp >= 0
    if n and on.any():
        roots, size = np.unique(comp[on], return_counts=True)  # ascending root = raster order
        root_lab = lab.reshape(-1)[roots].astype(np.int64)
        kept = np.full(n, -1, dtype=np.int64)
        for k in np.unique(root_lab):
            sel = np.nonzero(root_lab == k)[0]
            j = sel[np.argmax(size[sel])]  # the first maximum: raster-first on ties
            kept[k], areas[k] = roots[j], size[j]
        keep = on & (comp == kept[np.where(on, lab, 0)])
        cleaned[keep] = lab[keep]
        ys, xs = np.nonzero(keep)
        kl = lab[ys, xs].astype(np.int64)
        y0, x0 = np.full(n, h), np.full(n, w)
        y1, x1 = np.full(n, -1), np.full(n, -1)
        np.minimum.at(y0, kl, ys), np.minimum.at(x0, kl, xs), np.maximum.at(y1, kl, ys), np.maximum.at(x1, kl, xs)
        for k in np.nonzero(kept >= 0)[0]:
            if y1[k] - y0[k] < 2 or x1[k] - x0[k] < 2:
                continue
            free = np.ones((y1[k] - y0[k] + 3, x1[k] - x0[k] + 3), dtype=bool)
            free[1:-1, 1:-1] = cleaned[y0[k] : y1[k] + 1, x0[k] : x1[k] + 1] != k
            c = _components(free.astype(np.int8) - 1)
            hy, hx = np.nonzero(free & (c != c[0, 0]))  # (the ring is free and connected: one component, which holds the corner)
            if len(hy):
                holes.append(np.stack([(hy + y0[k] - 1) * w + (hx + x0[k] - 1), np.full(len(hy), k)], axis=1).astype(np.int32))
                areas[k] += len(hy)
    return cleaned, (np.concatenate(holes) if holes else np.zeros((0, 2), np.int32)), areas


def _group_host(fg, hm, off, fg_threshold, peak_threshold, output_stride, max_instances, center_nms_kernel, distance_gate_alpha, distance_gate_iters,
                mask_cleanup: bool = False, merge: Optional[dict] = None, merge_trace: Optional[list] = None) -> Grouping:
    B, _c, h, w = fg.shape
    labels = np.full((B, h, w), -1, dtype=np.int32)
    centers, scores, counts = [], [], []
    holes = [] if mask_cleanup else None
    s = output_stride
    for b in range(B):
        cen, val = find_center_peaks_host(hm[b, 0], peak_threshold, center_nms_kernel)
        if max_instances is not None and len(cen) > int(max_instances):
            order = np.lexsort((np.arange(len(val)), -val.astype(np.float64)))[: int(max_instances)]  # descending value, the earlier component first
            cen, val = cen[order], val[order]
        cnt = np.zeros(len(cen), dtype=np.int64)
        mask = fg[b, 0] > fg_threshold
        if len(cen) and bool(mask.any()):
            yx = torch.nonzero(mask, as_tuple=False)
            y, x = yx[:, 0], yx[:, 1]
            px = x.float() * s + s / 2.0 + off[b, 0][y, x]
            py = y.float() * s + s / 2.0 + off[b, 1][y, x]
            c = torch.from_numpy(cen)
            cx = c[:, 0].float() * s + s / 2.0
            cy = c[:, 1].float() * s + s / 2.0
            ddx, ddy = px[:, None] - cx[None], py[:, None] - cy[None]
            d = ddx * ddx + ddy * ddy
            assign = d.argmin(dim=1)
            dmin = d.gather(1, assign[:, None])[:, 0]
            keep = torch.ones_like(assign, dtype=torch.bool)
            if distance_gate_alpha is not None:
                for _ in range(max(1, int(distance_gate_iters))):
                    kept = torch.bincount(assign[keep], minlength=len(cen))
                    r = (float(distance_gate_alpha) * torch.sqrt(kept.float() / math.pi)) * float(s)
                    keep = dmin <= (r * r)[assign]
            lab = torch.where(keep, assign, torch.full_like(assign, -1))
            labels[b][y.numpy(), x.numpy()] = lab.numpy()
            cnt = torch.bincount(assign[keep], minlength=len(cen)).numpy()
        if mask_cleanup:
            labels[b], hol, cnt = clean_label_map(labels[b], len(cen))
            holes.append(hol)
        centers.append(cen)
        scores.append(val)
        counts.append(cnt.astype(np.int32))
    n_max = max([len(c) for c in centers] + [0])
    g = Grouping(labels.astype(_np_label_dtype(n_max)), centers, scores, counts, holes)
    if merge is not None:
        tables = []
        for b in range(B):
            _T, mom, edges, ridge = merge_tables_host(g.labels[b], hm[b, 0].numpy(), off[b].numpy(), centers[b], len(centers[b]), output_stride, merge["merge_dilate"])
            tables.append((edges, ridge, mom))
        g = merge_grouping(g, tables, output_stride, merge, trace=merge_trace)
    return g


def _merge_kw(merge_method, merge_thresholds, merge_w_valley, merge_w_offset, merge_dilate, join_bias) -> dict:
    return dict(merge_method=str(merge_method), merge_thresholds=tuple(float(t) for t in merge_thresholds), merge_w_valley=float(merge_w_valley),
                merge_w_offset=float(merge_w_offset), merge_dilate=int(merge_dilate), join_bias=float(join_bias))


def merge_grouping(g: Grouping, tables, output_stride: int, merge: dict, trace: Optional[list] = None) -> Grouping:
    """The fragment merge applied to a ``Grouping``: ``tables[b] = (edges (E, 4), ridge (E,), moments (n, 4))`` of frame b (``merge_tables_host`` or the
    device record), ``merge`` the ``merge_*`` knobs and ``join_bias``.  ``trace`` (a list) receives one dict per frame (``segmentation_merge.merge_frame``)."""
    labels = g.labels.copy()
    centers, scores, counts, members = [], [], [], []
    for b in range(labels.shape[0]):
        edges, ridge, mom = tables[b]
        tr = {} if trace is not None else None
        labels[b], c, s, n, m = merge_frame(labels[b], g.centers[b], g.scores[b], g.counts[b], edges, ridge, mom, output_stride, method=merge["merge_method"],
                                            thresholds=merge["merge_thresholds"], w_valley=merge["merge_w_valley"], w_offset=merge["merge_w_offset"],
                                            join_bias=merge["join_bias"], trace=tr)
        centers.append(c), scores.append(s), counts.append(n), members.append(m)
        if trace is not None:
            trace.append(tr)
    return Grouping(labels, centers, scores, counts, None, members)


def _np_label_dtype(n: int):
    return np.int8 if n <= 127 else (np.int16 if n <= 32767 else np.int32)


# ---- device implementation ----------------------------------------------------------------------------------------

# Pinned result buffers, recycled: at most _PINNED_KEYS (shape, dtype) kinds with up to two buffers each, the least recently used kind dropped first
# (a new batch shape or a retry with more room must not pin memory for good); one lock, so layers may be driven from several threads.
_PINNED_KEYS = 8
_pinned: "OrderedDict[tuple, list]" = OrderedDict()
_pinned_lock = threading.Lock()


def _pinned_take(shape, dtype) -> torch.Tensor:
    with _pinned_lock:
        free = _pinned.get((tuple(shape), dtype))
        if free:
            _pinned.move_to_end((tuple(shape), dtype))
            return free.pop()
    return torch.empty(tuple(shape), dtype=dtype, pin_memory=True)


def _pinned_give(t: torch.Tensor) -> None:
    key = (tuple(t.shape), t.dtype)
    with _pinned_lock:
        free = _pinned.setdefault(key, [])
        _pinned.move_to_end(key)
        if len(free) < 2:
            free.append(t)
        while len(_pinned) > _PINNED_KEYS:
            _pinned.popitem(last=False)


def group_enqueue(fg: torch.Tensor, hm: torch.Tensor, off: torch.Tensor, fg_threshold: float, peak_threshold: float, output_stride: int,
                  max_instances: Optional[int], center_nms_kernel: int, distance_gate_alpha: Optional[float], distance_gate_iters: int,
                  cap: int = DEFAULT_CAP, max_centers: int = DEFAULT_MAX_CENTERS, mask_cleanup: bool = False, hole_cap: int = DEFAULT_HOLE_CAP,
                  pool_words: Optional[int] = None, merge_fragments: bool = False, merge_method: str = "greedy", merge_thresholds: tuple = (0.85, 0.6, 0.4),
                  merge_w_valley: float = 1.0, merge_w_offset: float = 0.25, merge_dilate: int = 1, join_bias: float = 0.5,
                  edge_cap: int = DEFAULT_EDGE_CAP, merge_trace: Optional[list] = None) -> dict:
    """The grouping launches on the current stream and the asynchronous copies of their results into pinned memory; no host synchronisation.  With
    ``mask_cleanup`` ``ph_seg_cleanup`` follows the assignment / gate on the same stream; its record and hole list (``hole_cap`` pairs per frame,
    ``pool_words`` 64-bit words per frame for boxes beyond the LDS bitmaps: by default one box of the whole map) are copied with the rest.  With
    ``merge_fragments`` ``ph_seg_merge_tables`` follows the assignment / gate instead: its moments and edge list (``edge_cap`` pairs per frame) are copied
    with the rest as well -- still one event and one host read; without it the launches and copies are exactly those above."""
    from sleap_nn_amd import _lib as L

    merge = None
    if merge_fragments:
        if mask_cleanup:
            raise NotImplementedError("merge_fragments=True together with mask_cleanup=True is not built: see inference/ops/segmentation_merge.py")
        check_merge_args(merge_method, merge_dilate, device=True, max_centers=max_centers)
        merge = _merge_kw(merge_method, merge_thresholds, merge_w_valley, merge_w_offset, merge_dilate, join_bias)

    lib = L.lib()
    L.require_cuda(fg, "foreground")
    fg, hm, off = (t.detach().to(torch.float32).contiguous() for t in (fg, hm, off))
    B, _c, h, w = fg.shape
    if tuple(hm.shape) != (B, 1, h, w) or tuple(off.shape) != (B, 2, h, w) or _c != 1:
        raise ValueError(f"expected foreground (B, 1, h, w), centre (B, 1, h, w) and offsets (B, 2, h, w), got {tuple(fg.shape)}, {tuple(hm.shape)}, {tuple(off.shape)}")
    dev = fg.device
    gate = distance_gate_alpha is not None
    iters = max(1, int(distance_gate_iters)) if gate else 0
    mc = int(max_centers)
    ldt = label_dtype(mc)
    # one int32 record: [counts 2B | centres 2 B mc | scores B mc (fp32 bits) | pixel counts (iters + 1) B mc]
    n_small = 2 * B + 3 * B * mc + (iters + 1) * B * mc
    with torch.cuda.device(dev):
        small = torch.empty(n_small, dtype=torch.int32, device=dev)
        counts = small[: 2 * B]
        cen = small[2 * B : 2 * B + 2 * B * mc]
        sc = small[2 * B + 2 * B * mc : 2 * B + 3 * B * mc]
        pix = small[2 * B + 3 * B * mc :]
        need = int(lib.ph_seg_scratch_bytes(B, h, w, int(cap)))
        scratch = torch.empty((need + 7) // 8, dtype=torch.int64, device=dev)
        labels = torch.empty((B, h, w), dtype=ldt, device=dev)
        st = L.current_stream_ptr()
        p = lambda t: C.c_void_p(t.data_ptr())
        L.check(lib.ph_seg_center_peaks(p(hm), B, h, w, float(peak_threshold), int(center_nms_kernel), int(max_instances) if max_instances is not None else 0, int(cap), mc,
                                        p(cen), p(sc), p(counts), p(pix), iters + 1, p(scratch), need, st))
        dist = torch.empty((B, h, w), dtype=torch.float32, device=dev) if gate else None
        L.check(lib.ph_seg_assign(p(fg), p(off), B, h, w, float(fg_threshold), int(output_stride), p(cen), p(counts), mc, labels.element_size(), p(labels),
                                  p(dist) if gate else None, p(pix), st))
        if gate:
            gated = torch.empty_like(labels)
            L.check(lib.ph_seg_gate(p(labels), p(dist), B, h, w, float(distance_gate_alpha), int(output_stride), iters, p(counts), mc, labels.element_size(), p(pix),
                                    p(gated), st))
            labels = gated
        clean = None
        if mask_cleanup:
            hole_cap = max(1, int(hole_cap))
            pool_words = 2 * (h + 2) * ((w + 2 + 63) // 64) if pool_words is None else int(pool_words)
            rec = torch.empty(2 * B * mc + 2 * B, dtype=torch.int32, device=dev)  # [areas B mc | hole counts B mc | holes per frame B | pool words needed B]
            holes = torch.empty((B, hole_cap, 2), dtype=torch.int32, device=dev)
            cneed = int(lib.ph_seg_cleanup_scratch_bytes(B, h, w, mc, pool_words))
            cscratch = torch.empty((cneed + 7) // 8, dtype=torch.int64, device=dev)
            cleaned = torch.empty_like(labels)
            L.check(lib.ph_seg_cleanup(p(labels), B, h, w, p(counts), mc, labels.element_size(), p(cleaned), p(rec), p(holes), hole_cap, pool_words, p(cscratch),
                                       cneed, st))
            uncleaned, labels = labels, cleaned
            rec_h, holes_h = _pinned_take(rec.shape, rec.dtype), _pinned_take(holes.shape, holes.dtype)
            rec_h.copy_(rec, non_blocking=True)
            holes_h.copy_(holes, non_blocking=True)
            clean = {"rec": rec_h, "holes": holes_h, "hole_cap": hole_cap, "pool_words": pool_words, "dev": (rec, holes, cscratch, uncleaned)}
        if merge is not None:
            edge_cap = max(1, int(edge_cap))
            mom = torch.empty((B, mc, 4), dtype=torch.float64, device=dev)
            erec = torch.empty(B + B * edge_cap * 5, dtype=torch.int32, device=dev)  # [edges per frame B | edges (B, edge_cap, 5)]
            mneed = int(lib.ph_seg_merge_scratch_bytes(B, h, w, mc))
            mscratch = torch.empty((mneed + 7) // 8, dtype=torch.int64, device=dev)
            L.check(lib.ph_seg_merge_tables(p(labels), p(hm), p(off), B, h, w, int(output_stride), max(1, merge["merge_dilate"]), p(cen), p(counts), mc,
                                            labels.element_size(), p(mom), p(erec[:B]), p(erec[B:]), edge_cap, p(mscratch), mneed, st))
            mom_h, erec_h = _pinned_take(mom.shape, mom.dtype), _pinned_take(erec.shape, erec.dtype)
            mom_h.copy_(mom, non_blocking=True)
            erec_h.copy_(erec, non_blocking=True)
            merge = dict(merge, mom=mom_h, erec=erec_h, edge_cap=edge_cap, trace=merge_trace, dev=(mom, erec, mscratch))
        small_h = _pinned_take(small.shape, small.dtype)
        labels_h = _pinned_take(labels.shape, labels.dtype)
        small_h.copy_(small, non_blocking=True)
        labels_h.copy_(labels, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(dev))
    args = (fg, hm, off, fg_threshold, peak_threshold, output_stride, max_instances, center_nms_kernel, distance_gate_alpha, distance_gate_iters)
    return {"small": small_h, "labels": labels_h, "event": ev, "B": B, "mc": mc, "cap": int(cap), "iters": iters, "args": args, "dev": (small, labels, scratch, dist),
            "clean": clean, "merge": merge}


def group_finish(hd: dict) -> Grouping:
    """Wait for the batch's record (the one host read), come back with room when a frame had more candidates than ``cap`` or more centres than ``max_centers`` --
    or, with mask cleanup, more holes than ``hole_cap`` or large boxes beyond ``pool_words``, or, with the fragment merge, more touching pairs than ``edge_cap``.
    The merge's graph part runs here, on the host, from the record."""
    hd["event"].synchronize()
    B, mc, iters = hd["B"], hd["mc"], hd["iters"]
    small = hd["small"].numpy()
    n_cen, n_cand = small[:B], small[B : 2 * B]
    most_cand, most_cen = int(n_cand.max(initial=0)), int(n_cen.max(initial=0))
    cl = hd.get("clean")
    mg = hd.get("merge")
    give = [hd["small"], hd["labels"]] + ([cl["rec"], cl["holes"]] if cl else []) + ([mg["mom"], mg["erec"]] if mg else [])
    again = dict(merge_fragments=True, edge_cap=mg["edge_cap"], merge_trace=mg["trace"], **{k: mg[k] for k in MERGE_DEFAULTS}) if mg else {}
    if most_cand > hd["cap"] or most_cen > mc:  # rare (a frame that overflowed its candidate list reported no centres: it may come back once more for those)
        cap, mc2 = max(hd["cap"], most_cand), max(mc, most_cen)
        for t in give:
            _pinned_give(t)
        more = dict(mask_cleanup=True, hole_cap=cl["hole_cap"], pool_words=cl["pool_words"]) if cl else again
        return group_finish(group_enqueue(*hd["args"], cap=cap, max_centers=mc2, **more))
    if cl:
        rec = cl["rec"].numpy()
        n_holes, pool_need = rec[2 * B * mc : 2 * B * mc + B], rec[2 * B * mc + B :]
        most_holes, most_pool = int(n_holes.max(initial=0)), int(pool_need.max(initial=0))
        if most_holes > cl["hole_cap"] or most_pool > cl["pool_words"]:  # (an instance without pool room reported no holes: it may come back once more for those)
            for t in give:
                _pinned_give(t)
            return group_finish(group_enqueue(*hd["args"], cap=hd["cap"], max_centers=mc, mask_cleanup=True, hole_cap=max(cl["hole_cap"], most_holes),
                                              pool_words=max(cl["pool_words"], most_pool)))
    if mg:
        n_edges = mg["erec"].numpy()[:B]
        most_edges = int(n_edges.max(initial=0))
        if most_edges > mg["edge_cap"]:
            for t in give:
                _pinned_give(t)
            return group_finish(group_enqueue(*hd["args"], cap=hd["cap"], max_centers=mc, **dict(again, edge_cap=most_edges)))
    cen = small[2 * B : 2 * B + 2 * B * mc].reshape(B, mc, 2)
    sc = small[2 * B + 2 * B * mc : 2 * B + 3 * B * mc].view(np.float32).reshape(B, mc)
    pix = small[2 * B + 3 * B * mc :].reshape(iters + 1, B, mc)[iters]
    holes = None
    if cl:
        pix = rec[: B * mc].reshape(B, mc)  # the cleaned areas
        holes = [cl["holes"][b, : n_holes[b]].numpy().copy() for b in range(B)]
    out = Grouping(hd["labels"].numpy().copy(), [cen[b, : n_cen[b]].copy() for b in range(B)], [sc[b, : n_cen[b]].copy() for b in range(B)],
                   [pix[b, : n_cen[b]].copy() for b in range(B)], holes)
    if not cl and not mg:
        out.labels_dev = hd["dev"][1]
    if mg:
        er = mg["erec"].numpy()[B:].reshape(B, mg["edge_cap"], 5)
        mom = mg["mom"].numpy()
        tables = [(er[b, : n_edges[b], :4].astype(np.int64), er[b, : n_edges[b], 4].copy().view(np.float32), mom[b, : n_cen[b]].copy()) for b in range(B)]
        out = merge_grouping(out, tables, hd["args"][5], mg, trace=mg["trace"])
    for t in give:
        _pinned_give(t)
    return out


def group_instances_from_offsets(foreground: torch.Tensor, center_heatmap: torch.Tensor, offsets: torch.Tensor, fg_threshold: float = 0.5, peak_threshold: float = 0.2,
                                 output_stride: int = 2, max_instances: Optional[int] = None, center_nms_kernel: int = 3, distance_gate_alpha: Optional[float] = None,
                                 distance_gate_iters: int = 3, device=None, cap: int = DEFAULT_CAP, max_centers: int = DEFAULT_MAX_CENTERS, mask_cleanup: bool = False,
                                 hole_cap: int = DEFAULT_HOLE_CAP, pool_words: Optional[int] = None, merge_fragments: bool = False, merge_method: str = "greedy",
                                 merge_thresholds: tuple = (0.85, 0.6, 0.4), merge_w_valley: float = 1.0, merge_w_offset: float = 0.25, merge_dilate: int = 1,
                                 join_bias: float = 0.5, edge_cap: int = DEFAULT_EDGE_CAP, merge_trace: Optional[list] = None) -> Grouping:
    """``foreground`` (B, 1, h, w) probabilities, ``center_heatmap`` (B, 1, h, w), ``offsets`` (B, 2, h, w) = (dx, dy) -> ``Grouping``.  ``mask_cleanup``: keep each
    instance's largest component and fill its holes (``hole_cap`` / ``pool_words``: the device path's first capacities).  ``merge_fragments``: fuse
    touching fragments (``merge_instances`` with ``merge_method`` ``"greedy"`` / ``"multicut"`` / ``"none"``, the ``merge_*`` knobs and ``join_bias`` as there;
    ``edge_cap``: the device path's first capacity of touching pairs per frame; ``merge_dilate`` above 4 is a ``ValueError`` on the device; ``merge_trace``: a list that receives one dict per frame with the graph's ``"edges"``
    ``(i, j, affinity)``, their ``"detail"`` and the agglomeration's ``"decisions"``, centres numbered as before the merge).  ``device=None``: where the
    tensors are -- the HIP kernels for GPU tensors, the host implementation for CPU tensors; ``device="cuda..."`` moves CPU tensors to the GPU first, ``"cpu"`` the other way."""
    if center_nms_kernel not in (3, 5, 7):
        raise ValueError(f"center_nms_kernel must be 3, 5 or 7, got {center_nms_kernel}")
    dev = torch.device(device) if device is not None else foreground.device
    merge = None
    if merge_fragments:
        if mask_cleanup:
            raise NotImplementedError("merge_fragments=True together with mask_cleanup=True is not built: see inference/ops/segmentation_merge.py")
        check_merge_args(merge_method, merge_dilate, device=dev.type == "cuda", max_centers=max_centers)
        merge = _merge_kw(merge_method, merge_thresholds, merge_w_valley, merge_w_offset, merge_dilate, join_bias)
    if dev.type == "cuda":
        fg, hm, off = (t.to(dev) for t in (foreground, center_heatmap, offsets))
        more = dict(mask_cleanup=True, hole_cap=hole_cap, pool_words=pool_words) if mask_cleanup else {}
        if merge is not None:
            more = dict(merge_fragments=True, edge_cap=edge_cap, merge_trace=merge_trace, **merge)
        return group_finish(group_enqueue(fg, hm, off, fg_threshold, peak_threshold, output_stride, max_instances, center_nms_kernel, distance_gate_alpha,
                                          distance_gate_iters, cap=cap, max_centers=max_centers, **more))
    fg, hm, off = (t.detach().to("cpu", torch.float32) for t in (foreground, center_heatmap, offsets))
    return _group_host(fg, hm, off, fg_threshold, peak_threshold, output_stride, max_instances, center_nms_kernel, distance_gate_alpha, distance_gate_iters,
                       mask_cleanup=bool(mask_cleanup), merge=merge, merge_trace=merge_trace)


def semantic_enqueue(foreground: torch.Tensor, fg_threshold: float = 0.5, host_masks: bool = True) -> dict:
    """``ph_seg_semantic`` on the current stream and the asynchronous copies of its record (sums, counts) -- and, with ``host_masks``, of the 0 / 1
    maps -- into pinned memory; no host synchronisation.  ``mask_dev`` (B, h, w) uint8 stays on the device."""
    from sleap_nn_amd import _lib as L

    lib = L.lib()
    fg = L.require_cuda(foreground, "foreground").detach().to(torch.float32).contiguous()
    B, _c, h, w = fg.shape
    dev = fg.device
    with torch.cuda.device(dev):
        mask = torch.empty((B, h, w), dtype=torch.uint8, device=dev)
        rec = torch.empty(2 * B, dtype=torch.float64, device=dev)  # [sums B | counts B int32 in the first half of the second B doubles]
        cnt = rec[B:].view(torch.int32)[:B]
        need = int(lib.ph_seg_semantic_scratch_bytes(B, h, w))
        scratch = torch.empty((need + 7) // 8, dtype=torch.int64, device=dev)
        p = lambda t: C.c_void_p(t.data_ptr())
        L.check(lib.ph_seg_semantic(p(fg), B, h, w, float(fg_threshold), p(mask), p(cnt), p(rec), p(scratch), need, L.current_stream_ptr()))
        mask_h = _pinned_take(mask.shape, mask.dtype) if host_masks else None
        rec_h = _pinned_take(rec.shape, rec.dtype)
        if host_masks:
            mask_h.copy_(mask, non_blocking=True)
        rec_h.copy_(rec, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(dev))
    return {"mask_dev": mask, "mask": mask_h, "rec": rec_h, "event": ev, "B": B, "dev": (fg, rec, scratch)}


def semantic_finish(hd: dict):
    """Wait for the record of ``semantic_enqueue`` (the one host read): (masks (B, h, w) bool ndarray or None, pixel counts (B,), scores (B,))."""
    hd["event"].synchronize()
    B, rec_h, mask_h = hd["B"], hd["rec"], hd["mask"]
    sums = rec_h[:B].numpy().copy()
    counts = rec_h[B:].view(torch.int32)[:B].numpy().astype(np.int64)
    masks = None
    if mask_h is not None:
        masks = mask_h.numpy().astype(bool)
        _pinned_give(mask_h)
    _pinned_give(rec_h)
    return masks, counts, np.where(counts > 0, sums / np.maximum(counts, 1), 0.0)


def semantic_masks(foreground: torch.Tensor, fg_threshold: float = 0.5):
    """``foreground`` (B, 1, h, w) -> (masks (B, h, w) bool ndarray, pixel counts (B,), scores (B,) = mean probability over the mask, 0 where it is empty).
    GPU tensors: ``ph_seg_semantic`` (count and sum on the device, one byte per pixel to the host); CPU tensors: torch."""
    fg = foreground.detach().to(torch.float32).contiguous()
    B, _c, h, w = fg.shape
    if not fg.is_cuda:
        m = fg[:, 0] > fg_threshold
        cnt = m.flatten(1).sum(1).numpy()
        scores = np.array([float(fg[b, 0][m[b]].mean()) if cnt[b] else 0.0 for b in range(B)], dtype=np.float64)
        return m.numpy(), cnt.astype(np.int64), scores
    return semantic_finish(semantic_enqueue(fg, fg_threshold))


# ---- top-down crop masks: geometry and placement into frame space ---------------------------------------------------------------

class CropGeometry(NamedTuple):
    """Per crop: ``offset`` (N, 2) float64 (ox, oy) and ``scale`` (N, 2) float64 (sx, sy) as the ``pred_masks`` entries carry them
    (image = mask / scale + offset), ``origin`` (N, 2) int32 = round(offset) and ``extent`` (N, 2) int32 = (He, We), the decoded size."""

    offset: np.ndarray
    scale: np.ndarray
    origin: np.ndarray
    extent: np.ndarray


def mask_extent(mask_hw, scale) -> tuple:
    """``(He, We) = (round(h / sy), round(w / sx))``: the image extent a mask of ``mask_hw`` decodes to at ``scale = (sx, sy)``."""
    return int(round(mask_hw[0] / scale[1])), int(round(mask_hw[1] / scale[0]))


def crop_mask_geometry(topleft_sized, eff, input_scale: float, stride, crop_hw, mask_hw) -> CropGeometry:
    """Offset / scale of top-down crop masks in host arithmetic (layers/topdown_segmentation.py:232-271) and what their decoding needs.

    ``topleft_sized`` (N, 2) float32: the crop boxes' top-left corners (x, y) in sized space (``make_centered_bboxes``); the crop was cut at
    ``trunc(top_left + half) - half`` with ``half = (crop_w // 2, crop_h // 2)``, added in float32 like the gather.  ``eff`` (N,): the
    sizematcher scale of each crop's frame.  ``offset`` = that integer corner / eff, ``scale`` = eff * input_scale / stride (both axes)."""
    tl = np.asarray(topleft_sized, dtype=np.float32).reshape(-1, 2)
    eff = np.asarray(eff, dtype=np.float32).reshape(-1)
    n = tl.shape[0]
    ch, cw = int(crop_hw[0]), int(crop_hw[1])
    half = np.array([cw // 2, ch // 2], dtype=np.float32)
    corner = np.trunc(tl + half).astype(np.int64) - half.astype(np.int64)
    stride = float(stride)
    offset, scale = np.zeros((n, 2), np.float64), np.zeros((n, 2), np.float64)
    origin, extent = np.zeros((n, 2), np.int32), np.zeros((n, 2), np.int32)
    for k in range(n):
        e = float(eff[k])
        offset[k] = (float(corner[k, 0]) / e, float(corner[k, 1]) / e)
        scale[k] = ((e * float(input_scale)) / stride, (e * float(input_scale)) / stride)
        origin[k] = (int(round(offset[k, 0])), int(round(offset[k, 1])))
        extent[k] = mask_extent(mask_hw, scale[k])
    return CropGeometry(offset, scale, origin, extent)


def _place_host(masks: np.ndarray, pos: np.ndarray, origins: np.ndarray, extents: np.ndarray, H: int, W: int, P: int) -> np.ndarray:
    B = pos.shape[0] // P
    out = np.zeros((B, P, H, W), dtype=np.uint8)
    n, h, w = masks.shape
    for s in np.nonzero((pos >= 0) & (pos < n))[0]:
        k = int(pos[s])
        ox, oy = int(origins[k, 0]), int(origins[k, 1])
        He, We = int(extents[k, 0]), int(extents[k, 1])
        if not (1 <= He <= 65535 and 1 <= We <= 65535):
            continue
        y0, y1, x0, x1 = max(0, oy), min(H, oy + He), max(0, ox), min(W, ox + We)
        if y0 >= y1 or x0 >= x1:
            continue
        rows = ((np.arange(y0, y1, dtype=np.int64) - oy) * h) // He
        cols = ((np.arange(x0, x1, dtype=np.int64) - ox) * w) // We
        out[s // P, s % P, y0:y1, x0:x1] = masks[k][rows[:, None], cols[None, :]]
    return out


def place_crop_masks(masks, pos_of_slot, origins, extents, frame_hw, P: int):
    """Crop masks into frame space: ``uint8 (B, P, H, W)`` with ``B = len(pos_of_slot) // P`` -- the mask-stack form of ``evaluation.mask_pair_tables`` at stride 1.

    ``masks`` uint8 / bool (N, h, w) (or (N, 1, h, w)); ``pos_of_slot`` int32 (B * P,): the crop of each slot or -1; ``origins`` (N, 2) = (ox, oy) and
    ``extents`` (N, 2) = (He, We) integers (``crop_mask_geometry``).  Pixel (y, x) of a slot with crop k: ``v = y - oy, u = x - ox``; inside
    ``0 <= v < He`` and ``0 <= u < We`` it is ``masks[k, (v * h) // He, (u * w) // We]``, else 0 -- the nearest resample to the extent, the rounded
    origin, the top-left pad with negative rows / columns dropped and the clip to the frame of ``decode_mask_to_image_res``.
    GPU tensors: ``ph_seg_place_crops``, one launch on the current stream, no host synchronisation, the result stays on the device (``1 <= P <= 64``,
    fewer than 2^32 output bytes).  CPU tensors and arrays: NumPy, returned as an array (a tensor when ``masks`` is one)."""
    H, W = int(frame_hw[0]), int(frame_hw[1])
    P = int(P)
    on_gpu = torch.is_tensor(masks) and masks.is_cuda
    if P < 1 or (H < 1 or W < 1):
        raise ValueError(f"place_crop_masks: P={P} and the frame {H} x {W} must be positive")
    geom = np.concatenate([_host_int(origins).reshape(-1, 2), _host_int(extents).reshape(-1, 2)], axis=1) if not (torch.is_tensor(origins) and origins.is_cuda) else None
    if not on_gpu:
        m = masks.detach().numpy() if torch.is_tensor(masks) else np.asarray(masks)
        m = m.reshape((m.shape[0],) + tuple(m.shape[-2:])).astype(np.uint8)
        pos = _host_int(pos_of_slot).reshape(-1)
        if pos.shape[0] % P:
            raise ValueError(f"place_crop_masks: {pos.shape[0]} slots are no multiple of P={P}")
        out = _place_host(m, pos, geom[:, :2], geom[:, 2:], H, W, P)
        return torch.from_numpy(out) if torch.is_tensor(masks) else out
    from sleap_nn_amd import _lib as L

    dev = masks.device
    m = (masks.view(torch.uint8) if masks.dtype == torch.bool else masks.to(torch.uint8)).contiguous()
    n = int(m.shape[0])
    h, w = (int(m.shape[-2]), int(m.shape[-1])) if n else (1, 1)
    with torch.cuda.device(dev):
        pos = torch.as_tensor(pos_of_slot).to(dev, torch.int32, non_blocking=True).contiguous().view(-1)
        if pos.numel() % P:
            raise ValueError(f"place_crop_masks: {pos.numel()} slots are no multiple of P={P}")
        if geom is None:
            g = torch.cat([origins.view(-1, 2), torch.as_tensor(extents).to(dev).view(-1, 2)], dim=1).to(torch.int32).contiguous()
        else:
            g = torch.from_numpy(np.ascontiguousarray(geom, dtype=np.int32)).to(dev, non_blocking=True)
        if int(g.shape[0]) != n:
            raise ValueError(f"place_crop_masks: {n} masks, {int(g.shape[0])} geometry records")
        B = pos.numel() // P
        out = torch.empty((B, P, H, W), dtype=torch.uint8, device=dev)
        p = lambda t: C.c_void_p(t.data_ptr())
        L.check(L.lib().ph_seg_place_crops(p(m) if n else None, n, h, w, p(pos), p(g) if n else None, B, P, H, W, p(out), L.current_stream_ptr()))
    return out


def _host_int(x) -> np.ndarray:
    return (x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)).astype(np.int64)


def stack_pred_masks(pred_masks, frame_hw, P: Optional[int] = None):
    """Host ``pred_masks`` entries (any scale / offset) as a frame-space stack: ``(uint8 (B, P, H, W) ndarray, counts int32 (B,))``; slot j of a frame
    is its j-th entry, ``P`` defaults to the largest count (at least 1).  Every entry is decoded by ``place_crop_masks`` on its own extent."""
    B = len(pred_masks)
    counts = np.array([len(f) for f in pred_masks], dtype=np.int32)
    P = max(1, int(counts.max(initial=0))) if P is None else int(P)
    if int(counts.max(initial=0)) > P:
        raise ValueError(f"stack_pred_masks: a frame has {int(counts.max())} masks, P={P}")
    H, W = int(frame_hw[0]), int(frame_hw[1])
    out = np.zeros((B, P, H, W), dtype=np.uint8)
    for b, frame in enumerate(pred_masks):
        for j, d in enumerate(frame):
            m = np.asarray(d["mask"])
            scale, offset = d.get("scale", (1.0, 1.0)), d.get("offset", (0.0, 0.0))
            origin = np.array([[int(round(offset[0])), int(round(offset[1]))]])
            extent = np.array([mask_extent(m.shape, scale)])
            out[b, j] = _place_host(m[None].astype(np.uint8), np.zeros(1, np.int64), origin, extent, H, W, 1)[0, 0]
    return out, counts
