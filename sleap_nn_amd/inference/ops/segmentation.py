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
* a frame without foreground or without centres has no instances; instances left without pixels are dropped, the others keep their order.
"""
from __future__ import annotations

import ctypes as C
import math
import threading
from collections import OrderedDict
from dataclasses import dataclass
from typing import Dict, List, Optional

import numpy as np
import torch
import torch.nn.functional as F

DEFAULT_CAP = 2048  # candidates per frame that the collapse kernel keeps in LDS
DEFAULT_MAX_CENTERS = 127  # centres per frame that one-byte labels hold


@dataclass
class Grouping:
    """``labels`` (B, h, w) signed integers, -1 = background, otherwise an index into the frame's centres; per frame ``centers`` (N, 2) int32 (x, y) in map
    pixels, ``scores`` (N,) float32 (the centre's peak value) and ``counts`` (N,) the pixels each centre kept."""

    labels: np.ndarray
    centers: List[np.ndarray]
    scores: List[np.ndarray]
    counts: List[np.ndarray]

    def instances(self, b: int, output_stride: int) -> List[Dict]:
        """The reference's per-frame list (segmentation.py:213-237): ``{"mask", "center", "score"}`` per non-empty instance, in centre order; ``center`` in input pixels."""
        out = []
        lab = self.labels[b]
        s = np.float32(output_stride)
        half = np.float32(output_stride / 2.0)
        for k in np.nonzero(self.counts[b] > 0)[0]:
            cx, cy = self.centers[b][k]
            out.append({"mask": lab == k, "center": (float(np.float32(cx) * s + half), float(np.float32(cy) * s + half)), "score": float(self.scores[b][k])})
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


def _group_host(fg, hm, off, fg_threshold, peak_threshold, output_stride, max_instances, center_nms_kernel, distance_gate_alpha, distance_gate_iters) -> Grouping:
    B, _c, h, w = fg.shape
    labels = np.full((B, h, w), -1, dtype=np.int32)
    centers, scores, counts = [], [], []
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
        centers.append(cen)
        scores.append(val)
        counts.append(cnt.astype(np.int32))
    n_max = max([len(c) for c in centers] + [0])
    return Grouping(labels.astype(_np_label_dtype(n_max)), centers, scores, counts)


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
                  cap: int = DEFAULT_CAP, max_centers: int = DEFAULT_MAX_CENTERS) -> dict:
    """The grouping launches on the current stream and the asynchronous copies of their results into pinned memory; no host synchronisation."""
    from sleap_nn_amd import _lib as L

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
        small_h = _pinned_take(small.shape, small.dtype)
        labels_h = _pinned_take(labels.shape, labels.dtype)
        small_h.copy_(small, non_blocking=True)
        labels_h.copy_(labels, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(dev))
    args = (fg, hm, off, fg_threshold, peak_threshold, output_stride, max_instances, center_nms_kernel, distance_gate_alpha, distance_gate_iters)
    return {"small": small_h, "labels": labels_h, "event": ev, "B": B, "mc": mc, "cap": int(cap), "iters": iters, "args": args, "dev": (small, labels, scratch, dist)}


def group_finish(hd: dict) -> Grouping:
    """Wait for the batch's record (the one host read), come back with room when a frame had more candidates than ``cap`` or more centres than ``max_centers``."""
    hd["event"].synchronize()
    B, mc, iters = hd["B"], hd["mc"], hd["iters"]
    small = hd["small"].numpy()
    n_cen, n_cand = small[:B], small[B : 2 * B]
    most_cand, most_cen = int(n_cand.max(initial=0)), int(n_cen.max(initial=0))
    if most_cand > hd["cap"] or most_cen > mc:  # rare (a frame that overflowed its candidate list reported no centres: it may come back once more for those)
        cap, mc2 = max(hd["cap"], most_cand), max(mc, most_cen)
        _pinned_give(hd["small"])
        _pinned_give(hd["labels"])
        return group_finish(group_enqueue(*hd["args"], cap=cap, max_centers=mc2))
    cen = small[2 * B : 2 * B + 2 * B * mc].reshape(B, mc, 2)
    sc = small[2 * B + 2 * B * mc : 2 * B + 3 * B * mc].view(np.float32).reshape(B, mc)
    pix = small[2 * B + 3 * B * mc :].reshape(iters + 1, B, mc)[iters]
    out = Grouping(hd["labels"].numpy().copy(), [cen[b, : n_cen[b]].copy() for b in range(B)], [sc[b, : n_cen[b]].copy() for b in range(B)],
                   [pix[b, : n_cen[b]].copy() for b in range(B)])
    _pinned_give(hd["small"])
    _pinned_give(hd["labels"])
    return out


def group_instances_from_offsets(foreground: torch.Tensor, center_heatmap: torch.Tensor, offsets: torch.Tensor, fg_threshold: float = 0.5, peak_threshold: float = 0.2,
                                 output_stride: int = 2, max_instances: Optional[int] = None, center_nms_kernel: int = 3, distance_gate_alpha: Optional[float] = None,
                                 distance_gate_iters: int = 3, device=None, cap: int = DEFAULT_CAP, max_centers: int = DEFAULT_MAX_CENTERS) -> Grouping:
    """``foreground`` (B, 1, h, w) probabilities, ``center_heatmap`` (B, 1, h, w), ``offsets`` (B, 2, h, w) = (dx, dy) -> ``Grouping``.  ``device=None``: where the
    tensors are -- the HIP kernels for GPU tensors, the host implementation for CPU tensors; ``device="cuda..."`` moves CPU tensors to the GPU first, ``"cpu"`` the other way."""
    if center_nms_kernel not in (3, 5, 7):
        raise ValueError(f"center_nms_kernel must be 3, 5 or 7, got {center_nms_kernel}")
    dev = torch.device(device) if device is not None else foreground.device
    if dev.type == "cuda":
        fg, hm, off = (t.to(dev) for t in (foreground, center_heatmap, offsets))
        return group_finish(group_enqueue(fg, hm, off, fg_threshold, peak_threshold, output_stride, max_instances, center_nms_kernel, distance_gate_alpha,
                                          distance_gate_iters, cap=cap, max_centers=max_centers))
    fg, hm, off = (t.detach().to("cpu", torch.float32) for t in (foreground, center_heatmap, offsets))
    return _group_host(fg, hm, off, fg_threshold, peak_threshold, output_stride, max_instances, center_nms_kernel, distance_gate_alpha, distance_gate_iters)


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
    from sleap_nn_amd import _lib as L

    lib = L.lib()
    dev = fg.device
    with torch.cuda.device(dev):
        mask = torch.empty((B, h, w), dtype=torch.uint8, device=dev)
        rec = torch.empty(2 * B, dtype=torch.float64, device=dev)  # [sums B | counts B int32 in the first half of the second B doubles]
        cnt = rec[B:].view(torch.int32)[:B]
        need = int(lib.ph_seg_semantic_scratch_bytes(B, h, w))
        scratch = torch.empty((need + 7) // 8, dtype=torch.int64, device=dev)
        p = lambda t: C.c_void_p(t.data_ptr())
        L.check(lib.ph_seg_semantic(p(fg), B, h, w, float(fg_threshold), p(mask), p(cnt), p(rec), p(scratch), need, L.current_stream_ptr()))
        mask_h, rec_h = _pinned_take(mask.shape, mask.dtype), _pinned_take(rec.shape, rec.dtype)
        mask_h.copy_(mask, non_blocking=True)
        rec_h.copy_(rec, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(dev))
    ev.synchronize()
    sums = rec_h[:B].numpy().copy()
    counts = rec_h[B:].view(torch.int32)[:B].numpy().astype(np.int64)
    masks = mask_h.numpy().astype(bool)
    _pinned_give(mask_h)
    _pinned_give(rec_h)
    return masks, counts, np.where(counts > 0, sums / np.maximum(counts, 1), 0.0)
