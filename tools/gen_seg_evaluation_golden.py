"""Generate ``tests/golden/seg_evaluation.npz`` from the reference's own mask evaluation (``sleap_nn.evaluation`` through ``oracle.ref_harness``,
where the reference tree is available): ``_mask_pair_stats`` and ``match_masks`` on single frames, ``_mask_to_boundary`` / ``_boundary_iou``, and
``_process_frames_mask`` + ``mask_metrics`` + ``mask_voc_metrics`` and ``_process_frames_semantic`` + ``semantic_metrics`` on an ``Evaluator`` made
with ``object.__new__`` whose ``frame_pairs`` are stand-in frame objects (``_frame_masks`` / ``_frame_pred_scores`` / ``_union_frame_fg`` of that
module are pointed at the arrays the stand-ins hold; they only decode sleap-io masks).

Boundary IoU caveat: OpenCV is not installed where this runs and the harness's ``cv2`` stand-in is empty, so it is given ``BORDER_CONSTANT``,
``copyMakeBorder`` and ``erode`` written with NumPy / ``scipy.ndimage.binary_erosion(structure=ones((3, 3)), iterations=d, border_value=0)``.  The
boundary numbers are therefore pinned to the reference's code over that stand-in, not to OpenCV itself.  clDice: scikit-image is not installed either,
so the reference reports NaN, which is recorded as NaN.

Only data is recorded: the input masks bit-packed (``np.packbits``), counts, scores, and every returned array or number.

* ``pair/<case>/...``: (a) 4 frames on 37 x 53 with (P, G) = (3, 4), (0, 2), (2, 0), (5, 5): overlapping masks, an empty prediction, a pair with an
  empty union, a mask in a corner, tied scores; (b1) a 17 x 25 prediction at stride 2 under a 37 x 53 ground truth, (b2) over a 30 x 40 one;
  (c) P = G = 64 on 16 x 16 with single- and few-pixel masks; (d) one 200 x 300 frame of blobs.  Each with the results for the mask stack
  (``stack/``) and for the label map derived from it, lowest index first (``label/``).
* ``boundary/<case>/...``: the ground-truth masks of (a) (d = 1) and (d) (d = 7), and (d) at a dilation ratio of 0.05 (d = 18, wider than most blobs).
* ``ev/...``: 12 frames of blobs on 96 x 128 with label-map predictions at stride 2, in three batches of four.

Asserted here: (e) has an over-segmented ground-truth mask and an under-segmenting prediction and AP strictly between 0 and 1 at three thresholds or
more; no recorded IoU lies within 1e-9 of a threshold it is compared with (0.5 for the matching, the ten AP thresholds), and no coverage within 1e-9
of the fragmentation fraction.

    python tools/gen_seg_evaluation_golden.py
"""
from __future__ import annotations

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GOLD = os.path.join(ROOT, "tests", "golden")
MARGIN = 1e-9


def install():
    from oracle import ref_harness as rh

    rh.install()
    import scipy.ndimage as ndi

    cv2 = sys.modules["cv2"]
    cv2.BORDER_CONSTANT = 0

    def copy_make_border(src, top, bottom, left, right, border_type, value=0):
        assert border_type == cv2.BORDER_CONSTANT
        return np.pad(src, ((top, bottom), (left, right)), mode="constant", constant_values=value)

    def erode(src, kernel, iterations=1):
        return ndi.binary_erosion(src != 0, structure=kernel != 0, iterations=iterations, border_value=0).astype(src.dtype)

    cv2.copyMakeBorder, cv2.erode = copy_make_border, erode
    sys.modules["sleap_io"].PredictedInstance = type("PredictedInstance", (), {})
    import sleap_nn.evaluation as ev

    return ev


class Frame:
    def __init__(self, masks, scores=None):
        self.masks_, self.scores_ = masks, scores


def patch(ev):
    ev._frame_masks = lambda frame, drop_predicted_instances=False: list(frame.masks_)
    ev._frame_pred_scores = lambda frame: np.asarray(frame.scores_, dtype=float)

    def union(frame):
        if not frame.masks_:
            return np.zeros((1, 1), dtype=bool)
        h, w = max(m.shape[0] for m in frame.masks_), max(m.shape[1] for m in frame.masks_)
        canvas = np.zeros((h, w), dtype=bool)
        for m in frame.masks_:
            canvas[: m.shape[0], : m.shape[1]] |= m
        return canvas

    ev._union_frame_fg = union


def up(m, s):
    return np.repeat(np.repeat(m, s, axis=-2), s, axis=-1)


def ellipse(h, w, cy, cx, ry, rx):
    yy, xx = np.mgrid[0:h, 0:w]
    return ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0


def labels_of(stack, n):
    """Label map of a stack, lowest index first."""
    lab = np.full(stack.shape[1:], -1, np.int8)
    for p in range(n - 1, -1, -1):
        lab[stack[p]] = p
    return lab


def ragged(out, key, arrays, dtype):
    out[key + "_cat"] = np.concatenate([np.asarray(a, dtype=dtype).reshape(-1) for a in arrays]) if arrays else np.zeros(0, dtype)
    out[key + "_len"] = np.array([len(a) for a in arrays], np.int64)


def check_margin(iou, thresholds):
    iou = np.asarray(iou, dtype=float).reshape(-1, 1)
    if iou.size:
        assert np.abs(iou - np.asarray(thresholds, dtype=float).reshape(1, -1)).min() > MARGIN, "an IoU sits on a threshold"


def record_pair_case(ev, out, name, pred, gt, n_pred, n_gt, s):
    """pred (B, P, ph, pw) bool, gt (B, G, H, W) bool."""
    B, P = pred.shape[:2]
    G = gt.shape[1]
    k = f"pair/{name}/"
    out[k + "pred_bits"], out[k + "pred_shape"] = np.packbits(pred), np.array(pred.shape, np.int64)
    out[k + "gt_bits"], out[k + "gt_shape"] = np.packbits(gt), np.array(gt.shape, np.int64)
    out[k + "n_pred"], out[k + "n_gt"], out[k + "stride"] = np.asarray(n_pred, np.int32), np.asarray(n_gt, np.int32), np.int64(s)
    labels = np.stack([labels_of(pred[b], n_pred[b]) for b in range(B)])
    out[k + "labels"] = labels
    for form in ("stack", "label"):
        iou = np.full((B, P, G), np.nan)
        inter = np.zeros((B, P, G), np.int64)
        pa, ga = np.zeros((B, P), np.int64), np.zeros((B, G), np.int64)
        match = [[] for _ in range(5)]
        bious = []
        for b in range(B):
            pm = [up(pred[b, p], s) if form == "stack" else up(labels[b] == p, s) for p in range(n_pred[b])]
            gm = [gt[b, g] for g in range(n_gt[b])]
            i, n = ev._mask_pair_stats(pm, gm)
            iou[b, : n_pred[b], : n_gt[b]], inter[b, : n_pred[b], : n_gt[b]] = i, n
            pa[b, : n_pred[b]], ga[b, : n_gt[b]] = [int(m.sum()) for m in pm], [int(m.sum()) for m in gm]
            m5 = ev.match_masks(pm, gm, min_iou=0.5)
            check_margin(i, [0.5])
            for j in range(5):
                match[j].append(m5[j])
            bious.append([ev._boundary_iou(pm[int(p)], gm[int(g)]) for p, g in zip(m5[0], m5[1])])
        kk = k + form + "/"
        out[kk + "iou"], out[kk + "inter"], out[kk + "pred_area"], out[kk + "gt_area"] = iou, inter, pa, ga
        for j, nm in enumerate(("matched_pred", "matched_gt", "unmatched_pred", "unmatched_gt", "matched_ious")):
            ragged(out, kk + nm, match[j], np.float64 if j == 4 else np.int64)
        ragged(out, kk + "boundary_iou", bious, np.float64)


def record_boundary(ev, out, name, masks, ratio):
    h, w = masks.shape[1:]
    d = max(1, int(round(ratio * float(np.sqrt(h * h + w * w)))))
    bd = np.stack([ev._mask_to_boundary(m, ratio) for m in masks])
    k = f"boundary/{name}/"
    out[k + "mask_bits"], out[k + "shape"], out[k + "d"], out[k + "out_bits"] = np.packbits(masks), np.array(masks.shape, np.int64), np.int64(d), np.packbits(bd)
    return d, bd


def case_a(g):
    H, W = 37, 53
    gt, pred = np.zeros((4, 5, H, W), bool), np.zeros((4, 5, H, W), bool)
    # frame 0: (3, 4); ground truth 0 and 1 overlap; prediction 2 is empty and so is ground truth 3: their union is empty
    gt[0, 0], gt[0, 1], gt[0, 2] = ellipse(H, W, 10, 12, 6, 8), ellipse(H, W, 13, 20, 6, 7), ellipse(H, W, 28, 40, 5, 9)
    pred[0, 0], pred[0, 1] = ellipse(H, W, 10, 13, 6, 8), ellipse(H, W, 27, 41, 6, 8)
    # frame 1: (0, 2); frame 2: (2, 0)
    gt[1, 0], gt[1, 1] = ellipse(H, W, 8, 8, 4, 4), ellipse(H, W, 25, 30, 7, 5)
    pred[2, 0], pred[2, 1] = ellipse(H, W, 18, 26, 9, 9), ellipse(H, W, 20, 30, 5, 5)
    # frame 3: (5, 5); ground truth 0 touches the top and the left border, predictions 1 and 2 overlap
    gt[3, 0] = ellipse(H, W, 0, 0, 9, 11)
    pred[3, 0] = ellipse(H, W, 1, 0, 9, 10)
    for j, (cy, cx) in enumerate(((8, 30), (8, 45), (28, 12), (29, 36))):
        gt[3, j + 1] = ellipse(H, W, cy, cx, 5 + j % 2, 6)
        pred[3, j + 1] = ellipse(H, W, cy + int(g.integers(-2, 3)), cx + int(g.integers(-2, 3)), 5, 6 + j % 2)
    pred[3, 2] |= ellipse(H, W, 8, 36, 3, 4)
    scores = np.zeros((4, 5))
    scores[0, :3], scores[2, :2], scores[3] = (0.9, 0.7, 0.7), (0.5, 0.5), (0.8, 0.6, 0.95, 0.6, 0.3)
    return pred, gt, [3, 0, 2, 5], [4, 2, 0, 5], scores


def case_b(g, H, W):
    ph, pw, s = 17, 25, 2
    gt, pred = np.zeros((1, 3, H, W), bool), np.zeros((1, 3, ph, pw), bool)
    pred[0, 0], pred[0, 1], pred[0, 2] = ellipse(ph, pw, 5, 6, 3, 4), ellipse(ph, pw, 13, 20, 4, 5), ellipse(ph, pw, 14, 5, 3, 3)
    gt[0, 0], gt[0, 1], gt[0, 2] = ellipse(H, W, 10, 13, 7, 8), ellipse(H, W, 28, 41, 9, 12), ellipse(H, W, 27, 10, 6, 6)  # 1 crosses the smaller extent
    return pred, gt, [3], [3], s


def case_c(g):
    H = W = 16
    gt, pred = np.zeros((1, 64, H, W), bool), np.zeros((1, 64, H, W), bool)
    cells = g.permutation(H * W)
    for k in range(64):
        own = cells[4 * k : 4 * k + 1 + k % 4]  # one to four pixels
        gt[0, k].reshape(-1)[own] = True
        keep = own[: len(own) - (1 if len(own) >= 3 else 0)]  # IoU 1, 1, 2/3, 3/4: none on the matching threshold
        pred[0, 63 - k].reshape(-1)[keep] = True  # prediction 63 - k sits on ground truth k: bit 63 pairs with bit 0
    return pred, gt, [64], [64], 1


def case_d(g):
    H, W = 200, 300
    cen = [(30, 40, 4, 6), (60, 150, 5, 5), (100, 250, 3, 8), (150, 60, 6, 4), (170, 200, 5, 7), (40, 260, 4, 4), (110, 110, 24, 30), (185, 290, 6, 6)]
    gt, pred = np.zeros((1, len(cen), H, W), bool), np.zeros((1, len(cen), H, W), bool)
    for k, (cy, cx, ry, rx) in enumerate(cen):
        gt[0, k] = ellipse(H, W, cy, cx, ry, rx)
        pred[0, k] = ellipse(H, W, cy + int(g.integers(-1, 2)), cx + int(g.integers(-1, 2)), ry + (k % 2), rx)
    return pred, gt, [len(cen)], [len(cen)], 1


def case_e(g):
    """12 frames, ground truth on 96 x 128, label-map predictions on 48 x 64 at stride 2."""
    H, W, s, F, M = 96, 128, 2, 12, 6
    ph, pw = H // s, W // s
    gt, lab, scores = np.zeros((F, M, H, W), bool), np.full((F, ph, pw), -1, np.int8), np.zeros((F, M))
    n_pred, n_gt = [], []
    slots = [(20, 20), (20, 64), (20, 106), (70, 24), (70, 66), (72, 108)]
    for f in range(F):
        ng = [4, 5, 3, 6, 0, 4, 5, 2, 6, 3, 4, 5][f]
        n_gt.append(ng)
        order = g.permutation(len(slots))[:ng]
        preds = []
        for k, sl in enumerate(order):
            cy, cx = slots[sl]
            ry, rx = int(g.integers(8, 15)), int(g.integers(9, 17))
            gt[f, k] = ellipse(H, W, cy, cx, ry, rx)
            kind = (f + k) % 7
            if kind == 5:  # missed
                continue
            if kind == 3:  # split into a left and a right fragment
                preds.append(ellipse(ph, pw, cy / s, (cx - rx / 2) / s, ry / s, rx / 2 / s))
                preds.append(ellipse(ph, pw, cy / s, (cx + rx / 2) / s, ry / s, rx / 2 / s))
                continue
            jit = [0.0, 1.0, 2.5, 0, 4.0, 0, 6.0][kind]
            preds.append(ellipse(ph, pw, (cy + g.uniform(-jit, jit)) / s, (cx + g.uniform(-jit, jit)) / s, ry * g.uniform(0.8, 1.15) / s, rx * g.uniform(0.8, 1.15) / s))
        if f == 2 and ng >= 2:  # one prediction over the first two ground-truth masks
            preds = [up_ for up_ in preds[2:]] + [gt[f, 0][::s, ::s] | gt[f, 1][::s, ::s]]
        if f == 7:
            preds.append(ellipse(ph, pw, 40, 50, 3, 3))  # a false positive
        preds = preds[:M]
        for p in range(len(preds) - 1, -1, -1):
            lab[f][preds[p]] = p
        n_pred.append(len(preds))
        sc = np.round(g.uniform(0.3, 1.0, size=len(preds)), 1)  # one decimal: ties
        scores[f, : len(preds)] = sc
    return lab, gt, n_pred, n_gt, scores, s


def flatten(d, prefix, out):
    for k, v in d.items():
        if isinstance(v, dict):
            flatten(v, f"{prefix}{k}/", out)
        elif isinstance(v, str):
            out[prefix + k] = np.array(v)
        else:
            out[prefix + k] = np.asarray(v)


def main():
    ev = install()
    patch(ev)
    g = np.random.default_rng(20240611)
    out = {}

    pred, gt, n_pred, n_gt, scores = case_a(g)
    record_pair_case(ev, out, "a", pred, gt, n_pred, n_gt, 1)
    out["pair/a/scores"] = scores
    assert (gt[0, 0] & gt[0, 1]).any() and not pred[0, 2].any() and not gt[0, 3].any() and gt[3, 0][0, 0] and (pred[3, 1] & pred[3, 2]).any()
    d, _ = record_boundary(ev, out, "a", gt.reshape(-1, 37, 53), 0.02)
    assert d == 1
    for nm, (H, W) in (("b1", (37, 53)), ("b2", (30, 40))):
        pred, gt, n_pred, n_gt, s = case_b(g, H, W)
        record_pair_case(ev, out, nm, pred, gt, n_pred, n_gt, s)
    pred, gt, n_pred, n_gt, s = case_c(g)
    record_pair_case(ev, out, "c", pred, gt, n_pred, n_gt, s)
    assert (pred[0, 63] & gt[0, 0]).any()
    pred, gt, n_pred, n_gt, s = case_d(g)
    record_pair_case(ev, out, "d", pred, gt, n_pred, n_gt, s)
    d, bd = record_boundary(ev, out, "d", gt[0], 0.02)
    assert d == 7 and any((bd[k] != gt[0, k]).any() for k in range(len(bd))) and any((bd[k] == gt[0, k]).all() for k in range(len(bd)))
    d, bd = record_boundary(ev, out, "d_wide", gt[0], 0.05)
    assert d == 18

    # (e): the evaluator
    lab, gt, n_pred, n_gt, scores, s = case_e(g)
    F = len(n_pred)
    out["ev/labels"], out["ev/gt_bits"], out["ev/gt_shape"] = lab, np.packbits(gt), np.array(gt.shape, np.int64)
    out["ev/n_pred"], out["ev/n_gt"], out["ev/scores"], out["ev/stride"] = np.asarray(n_pred, np.int32), np.asarray(n_gt, np.int32), scores, np.int64(s)
    pairs = []
    for f in range(F):
        pairs.append((Frame([gt[f, k] for k in range(n_gt[f])]), Frame([up(lab[f] == p, s) for p in range(n_pred[f])], scores[f, : n_pred[f]])))
    e = object.__new__(ev.Evaluator)
    e.frame_pairs, e.match_threshold, e.exclude_predicted_instance_masks = pairs, 0.5, False
    e._process_frames_mask()
    mm, voc = e.mask_metrics(), e.mask_voc_metrics()
    assert mm["oversegmentation"] >= 1 and mm["undersegmentation"] >= 1, (mm["oversegmentation"], mm["undersegmentation"])
    ap = voc["mask_voc.AP"]
    assert np.count_nonzero((ap > 0.02) & (ap < 0.98)) >= 3 and len(np.unique(ap)) >= 3, ap
    for fr in e._mask_frames:
        check_margin(fr["iou"], list(ev.MASK_IOU_THRESHOLDS))
        if fr["inter"].size:
            check_margin(fr["inter"] / np.maximum(fr["gt_areas"][None, :], 1.0), [0.1])
    assert np.isnan(mm["mean_cldice"])
    flatten(mm, "ev/mask_metrics/", out)
    flatten(voc, "ev/mask_voc_metrics/", out)
    e2 = object.__new__(ev.Evaluator)
    e2.frame_pairs = pairs
    e2._process_frames_semantic()
    sm = e2.semantic_metrics()
    assert sm["n_frames"] == F - 1 and np.isnan(sm["cldices"]).all()
    flatten(sm, "ev/semantic_metrics/", out)

    path = os.path.join(GOLD, "seg_evaluation.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes;", "AP", np.round(ap, 3), "over", mm["oversegmentation"], "under", mm["undersegmentation"], "matched", mm["n_matched"],
          "fp", mm["n_fp"], "fn", mm["n_fn"])


if __name__ == "__main__":
    main()
