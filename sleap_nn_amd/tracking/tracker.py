"""``Tracker``: identities across frames (sleap_nn/tracking/tracker.py:50-628, candidates/fixed_window.py, candidates/local_queues.py, track_instance.py and
the parts of tracking/utils.py they use), on arrays.

``track(instances, frame_idx)`` takes one frame -- ``(I, N, 2)`` keypoints with NaN for missing nodes, or a list of ``pred_masks`` entries -- and returns
``(track_ids int64 (I,), tracking_scores float64 (I,))``, -1 / NaN for an instance left without a track (culled, below ``min_new_track_points``, beyond
``max_tracks``).  ``track_outputs(outputs)`` tracks a whole ``Outputs`` batch in ``frame_indices`` order.

Without a motion model a candidate's feature is the feature of the past instance itself, so every number the scoring needs is a function of one (current
instance, past instance) pair and none depends on a track assignment.  ``track_outputs`` therefore computes ALL pair scores of the batch first, in one native
call, and only the reduction per track, the matching and the queue update run frame by frame, on matrices of tens of entries:

* poses: ``ph_track_pose_scores`` (csrc/track_host.cpp), the batch against itself and the last ``min(window_size, 32)`` calls, float64 on the host;
* masks: ``ph_track_mask_pairs`` (csrc/track_kernels.hip) on the DEVICE label maps: weighted contingency tables of the batch against itself and a device ring
  of the last ``min(window_size, 32)`` label maps, integer sums, one device-to-host copy per batch.

Which layer takes which mask path.  The device tables need ``Outputs.pred_label_map`` (``SegmentationLayer(keep_label_map=True)``, which ``Predictor`` sets
when a tracker is configured): the plain bottom-up ``SegmentationLayer``, with or without ``full_res_masks``, as long as the frame geometry (map size, original
size, scale: the axis weights) stays what the ring holds and no frame has a label at or beyond 64.  The host function on the ``pred_masks`` bool arrays gives
the same numbers, only slower, and is used for ``CleanupSegmentationLayer`` (cleaned masks overlap: the label map no longer carries membership),
``MergeSegmentationLayer``, the top-down ``TopDownSegmentationLayer`` and ``SemanticSegmentationLayer`` (none hands a label map on), for a frame whose geometry
differs from the ring's, for a ``local_queues`` candidate older than the table's lags, and by ``track()`` itself.

The reference's quirks decide the ids and are kept: the fixed window's ``current_tracks`` is ``list(set(...))``, re-read inside ``update_tracks``' loop; its
queue only starts at the first frame that spawns a track; ``local_queues`` assigns the COLUMN INDEX as the track id; new ids are ``max + 1``; the pre-cull's
list handling (``cull_frame_instances``) is ported as it is, duplicates and all (an entry that appears twice is tracked twice; the later assignment wins).

Refused (``NotImplementedError`` naming the knob): ``use_flow`` (OpenCV's pyramidal LK), ``use_kalman`` (pykalman's EM), ``features="image"``.
"""
from __future__ import annotations

import warnings
from collections import defaultdict, deque
from dataclasses import replace
from typing import Any, Dict, List, Optional, Sequence, Tuple

import numpy as np

from sleap_nn_amd.tracking import scoring as S

_FEATURES = {"keypoints": S.keypoints_feature, "centroids": S.centroid_feature, "bboxes": S.bbox_feature, "masks": S.mask_feature}
_SCORES = ("oks", "iou", "mask_iou", "cosine_sim", "euclidean_dist")
_REDUCTIONS = ("mean", "max", "robust_quantile")
_MATCHING = ("hungarian", "greedy")
SAME_POSE_TOLERANCE = 5.0


class _Entry:
    """One instance of one call: ``src`` (keypoints or the mask entry), its feature, its support (non-NaN nodes, or mask area in image pixels), where the pair
    tables hold it (``call``, ``slot``), its row in the caller's input (``index``) and its detection score (the pre-cull sorts by it)."""

    __slots__ = ("src", "feature", "support", "call", "slot", "index", "score", "track_id", "tracking_score")

    def __init__(self, src, feature, support, call, slot, index, score):
        self.src, self.feature, self.support, self.call, self.slot, self.index, self.score = src, feature, support, call, slot, index, score
        self.track_id: Optional[int] = None
        self.tracking_score: Optional[float] = None

    def again(self) -> "_Entry":
        return _Entry(self.src, self.feature, self.support, self.call, self.slot, self.index, self.score)


class _Frame:
    """``TrackInstances``: the fixed window's queue item, parallel lists."""

    def __init__(self, entries: List[_Entry], frame_idx):
        self.entries = entries
        self.track_ids: List[Optional[int]] = [None] * len(entries)
        self.tracking_scores: List[Optional[float]] = [None] * len(entries)
        self.frame_idx = frame_idx


# ---- matching (utils.py:10-44) --------------------------------------------------------------------------------------

def hungarian_matching(cost: np.ndarray):
    """``linear_sum_assignment`` (the project's ``ph_lsap``) after the reference's fill of non-finite entries with ``10 max|finite| + 1`` (1e6 when none is finite)."""
    from sleap_nn_amd.inference.ops.paf import linear_sum_assignment

    invalid = ~np.isfinite(cost)
    if invalid.any():
        cost = np.copy(cost)
        finite = cost[~invalid]
        cost[invalid] = (np.abs(finite).max() * 10 + 1) if finite.size > 0 else 1e6
    if cost.shape[0] == 0 or cost.shape[1] == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    return linear_sum_assignment(cost)


def greedy_matching(cost: np.ndarray):
    rows, cols = np.unravel_index(np.argsort(cost, axis=None), cost.shape)
    edges = list(zip(rows, cols))
    row_inds, col_inds = [], []
    while edges:
        r, c = edges.pop(0)
        row_inds.append(r)
        col_inds.append(c)
        edges = [e for e in edges if e[0] != r and e[1] != c]
    return row_inds, col_inds


# ---- pre-cull (utils.py:255-341, 405-460) ---------------------------------------------------------------------------

def same_pose_as(a: np.ndarray, b: np.ndarray, tolerance: float = SAME_POSE_TOLERANCE) -> bool:
    """``PredictedInstance.same_pose_as``: every node visible in both lies within ``tolerance`` pixels; no common node is no match."""
    valid = ~(np.isnan(a).any(axis=1) | np.isnan(b).any(axis=1))
    if not valid.any():
        return False
    return bool(np.all(np.linalg.norm(a[valid] - b[valid], axis=1) <= tolerance))


def nms_fast(boxes: np.ndarray, scores: np.ndarray, iou_threshold: float, target_count: Optional[int] = None) -> list:
    if len(boxes) == 0:
        return []
    if target_count and len(boxes) < target_count:
        return list(range(len(boxes)))
    if boxes.dtype.kind == "i":
        boxes = boxes.astype("float")
    picked, removed = [], []
    x1, y1, x2, y2 = boxes[:, 0], boxes[:, 1], boxes[:, 2], boxes[:, 3]
    area = (x2 - x1 + 1) * (y2 - y1 + 1)
    idxs = np.argsort(scores)
    while len(idxs) > 0:
        best = idxs[-1]
        picked.append(best)
        rest = idxs[:-1]
        w = np.maximum(0, np.minimum(x2[best], x2[rest]) - np.maximum(x1[best], x1[rest]) + 1)
        h = np.maximum(0, np.minimum(y2[best], y2[rest]) - np.maximum(y1[best], y1[rest]) + 1)
        over = np.where((w * h) / area[rest] > iou_threshold)[0]
        removed.extend(list(idxs[over]))
        idxs = np.delete(idxs, over)[:-1]
    if target_count and removed and len(picked) < target_count:
        removed.sort(key=lambda i: -scores[i])
        picked.extend(removed[: min(len(removed), len(picked) - target_count)])  # (the reference's count: negative, so all but that many of the tail)
    return picked


def cull_frame_instances(entries: List[_Entry], instance_count: int, iou_threshold: Optional[float] = None) -> List[_Entry]:
    """The reference's per-frame cull as it is written, on entries; an entry the result names twice comes back twice."""
    if not entries:
        return entries  # (the reference returns None here and fails in the caller)
    out = entries
    if len(entries) > instance_count:
        keep = entries
        if iou_threshold:
            boxes = np.array([S.bbox_feature(e.src) for e in entries])
            scores = np.array([e.score for e in entries])
            picks = nms_fast(boxes, scores, iou_threshold, instance_count)
            keep = [e for i, e in enumerate(entries) if i in picks]
            extra = [e for i, e in enumerate(entries) if i not in picks]
            out = [e for x in extra for e in entries if not same_pose_as(e.src, x.src)]
        if len(keep) > instance_count:
            extra = sorted(keep, key=lambda e: e.score)[:-instance_count]
            out = [e for x in extra for e in out if same_pose_as(e.src, x.src)]
    seen, res = set(), []
    for e in out:  # one record per appearance: the same instance may be tracked twice
        res.append(e.again() if id(e) in seen else e)
        seen.add(id(e))
    return res


# ---- candidate makers -----------------------------------------------------------------------------------------------

class FixedWindowCandidates:
    def __init__(self, window_size: int = 5, min_new_track_points: int = 0):
        self.window_size, self.min_new_track_points = window_size, min_new_track_points
        self.tracker_queue: deque = deque(maxlen=window_size)
        self.all_tracks: List[int] = []

    @property
    def current_tracks(self) -> list:
        if not len(self.tracker_queue):
            return []
        cur = set()
        for fr in self.tracker_queue:
            cur.update(fr.track_ids)
        return list(cur)

    def make(self, entries: List[_Entry], frame_idx) -> _Frame:
        return _Frame(entries, frame_idx)

    def candidates_of(self, track_id) -> List[_Entry]:
        out = []
        for fr in self.tracker_queue:
            if track_id in fr.track_ids:
                out.append(fr.entries[fr.track_ids.index(track_id)])
        return out

    def add_new_tracks(self, cur: _Frame, add_to_queue: bool = True) -> _Frame:
        new = False
        for i, e in enumerate(cur.entries):
            if e.support > self.min_new_track_points and cur.track_ids[i] is None:
                new = True
                tid = 0 if not self.all_tracks else max(self.all_tracks) + 1
                cur.track_ids[i], cur.tracking_scores[i] = tid, 1.0
                self.all_tracks.append(tid)
        if add_to_queue and new:
            self.tracker_queue.append(cur)
        return cur

    def update_tracks(self, cur: _Frame, row_inds, col_inds, tracking_scores) -> _Frame:
        for k, (row, col) in enumerate(zip(row_inds, col_inds)):
            cur.track_ids[row] = self.current_tracks[col]
            cur.tracking_scores[row] = tracking_scores[k]
        self.tracker_queue.append(cur)
        if [x for x in range(len(cur.entries)) if x not in row_inds]:
            cur = self.add_new_tracks(cur, add_to_queue=False)
        return cur

    def results(self, cur: _Frame):
        return [(e.index, cur.track_ids[i], cur.tracking_scores[i]) for i, e in enumerate(cur.entries) if cur.track_ids[i] is not None]


class LocalQueueCandidates:
    def __init__(self, window_size: int = 5, max_tracks: Optional[int] = None, min_new_track_points: int = 0):
        self.window_size, self.max_tracks, self.min_new_track_points = window_size, max_tracks, min_new_track_points
        self.tracker_queue: Dict[int, deque] = defaultdict(deque)
        self.current_tracks: List[int] = []

    def make(self, entries: List[_Entry], frame_idx) -> List[_Entry]:
        return entries

    def candidates_of(self, track_id) -> List[_Entry]:
        return list(self.tracker_queue[track_id])

    def _new_track_id(self) -> Optional[int]:
        if not self.current_tracks:
            tid = 0
        else:
            tid = max(self.current_tracks) + 1
            if self.max_tracks is not None and tid >= self.max_tracks:
                return None
        self.tracker_queue[tid] = deque(maxlen=self.window_size)
        return tid

    def add_new_tracks(self, cur: List[_Entry]) -> List[_Entry]:
        out = []
        for e in cur:
            if e.support > self.min_new_track_points:
                tid = self._new_track_id()
                if tid is None:
                    continue
                e.track_id, e.tracking_score = tid, 1.0
                self.current_tracks.append(tid)
                self.tracker_queue[tid].append(e)
            out.append(e)
        return out

    def update_tracks(self, cur: List[_Entry], row_inds, col_inds, tracking_scores) -> List[_Entry]:
        res = []
        for k, (row, col) in enumerate(zip(row_inds, col_inds)):
            cur[row].track_id = int(col)  # (the column index IS the id: current_tracks is 0, 1, 2, ... in creation order)
            cur[row].tracking_score = tracking_scores[k]
            res.append(cur[row])
        for e in cur:
            if e.track_id is not None:
                self.tracker_queue[e.track_id].append(e)
        for ind in [x for x in range(len(cur)) if x not in row_inds]:
            res.extend(self.add_new_tracks([cur[ind]]))
        return [e for e in res if e.track_id is not None]

    def results(self, cur: List[_Entry]):
        return [(e.index, e.track_id, e.tracking_score) for e in cur if e.track_id is not None]


class _Table:
    """Pair scores of one frame of a batch: ``scores[k - 1][slot_cur][slot_past]`` for the frame k calls earlier, ``valid[k - 1]`` where the table reaches."""

    def __init__(self, scores: np.ndarray, valid: np.ndarray):
        self.scores, self.valid = scores, valid


class Tracker:
    def __init__(self, candidate, min_match_points: int = 0, features: str = "keypoints", scoring_method: str = "oks", scoring_reduction: str = "mean",
                 track_matching_method: str = "hungarian", robust_best_instance: float = 1.0, oks_stddev: float = 0.025, is_local_queue: bool = False,
                 tracking_target_instance_count: Optional[int] = None, tracking_pre_cull_to_target: int = 0, tracking_pre_cull_iou_threshold: float = 0) -> None:
        self.candidate = candidate
        self.min_match_points = min_match_points
        self.features, self.scoring_method, self.scoring_reduction = features, scoring_method, scoring_reduction
        self.track_matching_method, self.robust_best_instance, self.oks_stddev = track_matching_method, robust_best_instance, oks_stddev
        self.is_local_queue = is_local_queue
        self.tracking_target_instance_count = tracking_target_instance_count
        self.tracking_pre_cull_to_target = tracking_pre_cull_to_target
        self.tracking_pre_cull_iou_threshold = tracking_pre_cull_iou_threshold
        self.use_flow = False
        self.n_calls = 0  # calls of track so far: a past instance's lag is counted in calls
        self.last_scores: Optional[np.ndarray] = None  # get_scores' matrix of the last call (None when the queue was empty)
        self.table_hits = 0  # pair scores read from a table / computed pair by pair
        self.pair_calls = 0
        self._pose_hist: Optional[np.ndarray] = None  # (L, I, D / 2, 2) features of the last calls, newest last
        self._pose_counts: Optional[np.ndarray] = None
        self._pose_n_hist = 0
        self._mask_ring = None  # dict: device ring of label maps, newest last, with areas and geometry on the host

    @classmethod
    def from_config(cls, window_size: int = 5, min_new_track_points: int = 0, candidates_method: str = "fixed_window", min_match_points: int = 0,
                    features: str = "keypoints", scoring_method: str = "oks", scoring_reduction: str = "mean", robust_best_instance: float = 1.0,
                    oks_stddev: Optional[float] = None, track_matching_method: str = "hungarian", max_tracks: Optional[int] = None, use_flow: bool = False,
                    of_img_scale: float = 1.0, of_window_size: int = 21, of_max_levels: int = 3, use_kalman: bool = False, kf_track_features: str = "centroid",
                    kf_init_frame_count: int = 10, kf_node_indices: Optional[List[int]] = None, kf_reset_gap_size: int = 5, kf_prediction_blend: float = 0.5,
                    kf_gate_step_mult: float = 8.0, kf_min_gate_px: float = 40.0, kf_velocity_cap_mult: float = 3.0, kf_min_velocity_cap_px: float = 15.0,
                    tracking_target_instance_count: Optional[int] = None, tracking_pre_cull_to_target: int = 0,
                    tracking_pre_cull_iou_threshold: float = 0) -> "Tracker":
        """The reference's signature and defaults (tracker.py:128-158).  ``max_tracks`` with ``fixed_window`` switches to ``local_queues`` (the only maker that
        honours the cap); ``oks_stddev=None`` resolves to 0.025."""
        if max_tracks is not None and candidates_method == "fixed_window":
            candidates_method = "local_queues"
        if candidates_method == "fixed_window":
            candidate, local = FixedWindowCandidates(window_size=window_size, min_new_track_points=min_new_track_points), False
        elif candidates_method == "local_queues":
            candidate, local = LocalQueueCandidates(window_size=window_size, max_tracks=max_tracks, min_new_track_points=min_new_track_points), True
        else:
            raise ValueError(f"{candidates_method} is not a valid method. Please choose one of [`fixed_window`, `local_queues`]")
        if use_kalman and use_flow:
            raise ValueError("`use_kalman` and `use_flow` are mutually exclusive; choose one tracker (Kalman tracking does not use optical flow).")
        if use_flow:
            raise NotImplementedError("use_flow=True is not built on the MI355X path (OpenCV's pyramidal Lucas-Kanade flow): see sleap_nn_amd/tracking/tracker.py")
        if use_kalman:
            raise NotImplementedError("use_kalman=True is not built on the MI355X path (pykalman's EM fit): see sleap_nn_amd/tracking/tracker.py")
        if features == "image":
            raise NotImplementedError("features='image' is not built on the MI355X path: see sleap_nn_amd/tracking/tracker.py")
        if oks_stddev is None:
            oks_stddev = 0.025
        return cls(candidate=candidate, min_match_points=min_match_points, features=features, scoring_method=scoring_method, scoring_reduction=scoring_reduction,
                   robust_best_instance=robust_best_instance, oks_stddev=oks_stddev, track_matching_method=track_matching_method, is_local_queue=local,
                   tracking_target_instance_count=tracking_target_instance_count, tracking_pre_cull_to_target=tracking_pre_cull_to_target,
                   tracking_pre_cull_iou_threshold=tracking_pre_cull_iou_threshold)

    # -- one pair ---------------------------------------------------------------------------------------------------
    def _check(self) -> None:
        if self.features not in _FEATURES:
            raise ValueError("Invalid `features` argument. Please provide one of `keypoints`, `centroids`, `bboxes`, `masks` and `image`")
        if self.scoring_method not in _SCORES:
            raise ValueError("Invalid `scoring_method` argument. Please provide one of `oks`, `cosine_sim`, `iou`, `mask_iou`, and `euclidean_dist`.")
        if self.scoring_reduction not in _REDUCTIONS:
            raise ValueError("Invalid `scoring_reduction` argument. Please provide one of `mean`, `max`, and `robust_quantile`.")
        if self.track_matching_method not in _MATCHING:
            raise ValueError("Invalid `track_matching_method` argument. Please provide one of `hungarian`, and `greedy`.")

    def pair_score(self, a, b) -> float:
        """The NumPy score of a current feature against a past one."""
        m = self.scoring_method
        if m == "oks":
            return S.oks_score(a, b, self.oks_stddev)
        if m == "iou":
            return S.bbox_iou(a, b)
        if m == "mask_iou":
            return S.mask_iou(a, b)
        if m == "cosine_sim":
            return S.cosine_sim(a, b)
        return S.neg_euclidean(a, b)

    def _score(self, cur: _Entry, past: _Entry, table: Optional[_Table]) -> float:
        if table is not None:
            k = cur.call - past.call
            if 1 <= k <= len(table.valid) and table.valid[k - 1] and cur.slot >= 0 and past.slot >= 0:
                self.table_hits += 1
                return float(table.scores[k - 1, cur.slot, past.slot])
        self.pair_calls += 1
        return self.pair_score(self._feature(cur), self._feature(past))

    @staticmethod
    def _feature(e: _Entry):
        if e.feature is None:  # a mask entry the device tables covered so far: decoded only when a pair beyond their reach asks
            e.feature = S.mask_feature(e.src)
        return e.feature

    # -- one frame --------------------------------------------------------------------------------------------------
    def _entries(self, instances, instance_scores=None, slots=None, features=None, lazy: bool = False) -> List[_Entry]:
        self._check()
        masks = not isinstance(instances, np.ndarray) and len(instances) > 0 and isinstance(instances[0], dict)
        fn = _FEATURES[self.features]
        out = []
        for i in range(len(instances)):
            if masks and lazy and self.features == "masks":
                src, feat, support = instances[i], None, 0  # (feature on demand, support from the area table)
            elif masks:
                src = instances[i]
                feat = features[i] if features is not None else (S.mask_feature(src) if self.features == "masks" else None)
                if feat is None:
                    raise ValueError(f"features={self.features!r} cannot be computed from segmentation masks: use features='masks'")
                support = feat.area if isinstance(feat, S.MaskFeature) else S.mask_feature(src).area
            else:
                src = np.asarray(instances[i], dtype=np.float64)
                if self.features == "masks":
                    raise ValueError("features='masks' needs pred_masks entries, got keypoints")
                feat, support = fn(src), S.count_valid_points(src)
            sc = float(instance_scores[i]) if instance_scores is not None else (float(src.get("score", 0.0)) if masks else 0.0)
            out.append(_Entry(src, feat, support, self.n_calls, i if slots is None else int(slots[i]), i, sc))
        return out

    def _reduce(self, vals: list) -> float:
        if not vals:
            return np.nan
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", category=RuntimeWarning)
            if self.scoring_reduction == "mean":
                return np.nanmean(vals)
            if self.scoring_reduction == "robust_quantile":
                return np.nanquantile(vals, q=self.robust_best_instance)
            return np.nanmax(vals)

    def _track_entries(self, entries: List[_Entry], n: int, frame_idx, table: Optional[_Table] = None) -> Tuple[np.ndarray, np.ndarray]:
        masks = bool(entries) and isinstance(entries[0].src, dict)
        if not masks and self.tracking_target_instance_count and self.tracking_pre_cull_to_target:
            entries = cull_frame_instances(entries, self.tracking_target_instance_count, self.tracking_pre_cull_iou_threshold)
        cand = self.candidate
        cur = cand.make(entries, frame_idx)
        self.last_scores = None
        if cand.tracker_queue:
            tracks = cand.current_tracks
            past = {t: cand.candidates_of(t) for t in tracks}
            scores = np.zeros((len(entries), len(tracks)))
            for i, e in enumerate(entries):
                for j, t in enumerate(tracks):
                    scores[i][j] = self._reduce([self._score(e, p, table) for p in past[t] if p.support > self.min_match_points])
            self.last_scores = scores
            cost = -scores
            cost[np.isnan(cost)] = np.inf
            rows, cols = (hungarian_matching if self.track_matching_method == "hungarian" else greedy_matching)(cost)
            cur = cand.update_tracks(cur, rows, cols, [-cost[r, c] for r, c in zip(rows, cols)])
        else:
            cur = cand.add_new_tracks(cur)
        ids = np.full(n, -1, dtype=np.int64)
        tsc = np.full(n, np.nan, dtype=np.float64)
        for index, tid, score in cand.results(cur):
            ids[index], tsc[index] = tid, score
        self.n_calls += 1
        return ids, tsc

    def track(self, instances, frame_idx, instance_scores=None) -> Tuple[np.ndarray, np.ndarray]:
        """One frame, every score in NumPy.  ``instances``: ``(I, N, 2)`` keypoints (NaN = missing) or a list of ``pred_masks`` entries; ``instance_scores``
        ``(I,)``: the detection scores the pre-cull sorts by (a mask entry's ``"score"`` by default)."""
        ids, tsc = self._track_entries(self._entries(instances, instance_scores), len(instances), frame_idx)
        self._pose_hist, self._pose_n_hist, self._mask_ring = None, 0, None  # the tables' history does not hold this call: start it again
        return ids, tsc

    # -- a batch ----------------------------------------------------------------------------------------------------
    @property
    def table_lags(self) -> int:
        return max(1, min(int(self.candidate.window_size), S.MAX_TABLE_LAGS))

    def _pose_tables(self, frames: List[List[_Entry]], use_native: bool) -> List[Optional[_Table]]:
        """Features of the batch's entries into ``(B, I, N, 2)``, ``ph_track_pose_scores`` against the batch and the history, the history moved on."""
        B, L = len(frames), self.table_lags
        method = self.scoring_method
        if not use_native or method not in S.METHODS or not any(frames):
            self._pose_hist, self._pose_n_hist = None, 0
            return [None] * B
        first = np.asarray(next(e for fr in frames for e in fr).feature)
        D = first.size
        if D % 2 or (method == "iou" and D != 4) or (method == "cosine_sim" and first.ndim != 1):  # (shapes the NumPy functions refuse: let them)
            self._pose_hist, self._pose_n_hist = None, 0
            return [None] * B
        I = max(len(fr) for fr in frames)
        hist, hcounts, n_hist = self._pose_hist, self._pose_counts, self._pose_n_hist
        if hist is None or hist.shape[2] != D // 2 or hist.shape[0] != L:
            hist, hcounts, n_hist = np.zeros((L, I, D // 2, 2)), np.zeros(L, np.int32), 0
        if hist.shape[1] < I:
            hist = np.concatenate([hist, np.zeros((L, I - hist.shape[1], D // 2, 2))], axis=1)
        I = hist.shape[1]
        cur = np.full((B, I, D // 2, 2), np.nan)
        counts = np.zeros(B, np.int32)
        for b, fr in enumerate(frames):
            for s, e in enumerate(fr):
                e.slot = s
                cur[b, s] = np.asarray(e.feature, dtype=np.float64).reshape(D // 2, 2)
            counts[b] = len(fr)
        sc = S.pose_pair_scores(cur, hist, n_hist, np.concatenate([counts, hcounts]), method, self.oks_stddev)
        tables = [_Table(sc[b], np.array([(b >= k) or (k - b <= n_hist) for k in range(1, L + 1)])) for b in range(B)]
        self._pose_hist = np.concatenate([hist, cur])[-L:]
        self._pose_counts = np.concatenate([hcounts, counts])[-L:]
        self._pose_n_hist = min(L, n_hist + B)
        return tables

    def _mask_tables(self, outputs, order: Sequence[int], frames: List[List[_Entry]]) -> List[Optional[_Table]]:
        """``ph_track_mask_pairs`` on the batch's device label maps against the batch and the ring; None per frame where the host scores apply."""
        import torch

        B, L = len(frames), self.table_lags
        lm, labs, wts = outputs.pred_label_map, outputs.pred_mask_labels, outputs.pred_label_weights
        ok = self.scoring_method == "mask_iou" and lm is not None and labs is not None and wts is not None and lm.is_cuda
        if ok:
            rw, cw = wts[order[0]]
            ok = all(np.array_equal(wts[b][0], rw) and np.array_equal(wts[b][1], cw) for b in order)
            top = max([int(max(labs[b], default=-1)) for b in order])
            ok = ok and top < S.MAX_TABLE_LABELS and int(rw.sum()) * int(cw.sum()) < 2**31
        if not ok:
            self._mask_ring = None
            return [None] * B
        ring = self._mask_ring
        h, w = int(lm.shape[1]), int(lm.shape[2])
        if ring is None or ring["L"] != L or ring["hw"] != (h, w) or ring["dtype"] != lm.dtype or not (np.array_equal(ring["rw"], rw) and np.array_equal(ring["cw"], cw)):
            with torch.cuda.device(lm.device):
                ring = {"L": L, "hw": (h, w), "dtype": lm.dtype, "rw": rw, "cw": cw, "n": 0, "P": 8, "dev": torch.full((L, h, w), -1, dtype=lm.dtype, device=lm.device),
                        "areas": [None] * L, "rw_dev": torch.from_numpy(rw).to(lm.device), "cw_dev": torch.from_numpy(cw).to(lm.device)}
        P = ring["P"]
        while P <= top:
            P *= 2
        ring["P"] = P
        cur = lm if list(order) == list(range(lm.shape[0])) else lm.index_select(0, torch.as_tensor(list(order), device=lm.device))
        rec, _inter, _area = S.mask_pair_counts(cur, ring["dev"], ring["n"], ring["rw_dev"], ring["cw_dev"], P, int(rw.sum()) * int(cw.sum()))
        ring["dev"] = torch.cat([ring["dev"], cur])[-L:].contiguous()  # device to device, on the stream
        rec_h = rec.cpu().numpy()  # the one device-to-host copy of the batch
        inter = rec_h[: B * L * P * P].reshape(B, L, P, P)
        area = rec_h[B * L * P * P :].reshape(B, P)
        n_hist = ring["n"]
        tables = []
        for b in range(B):
            valid = np.array([(b >= k) or (k - b <= n_hist) for k in range(1, L + 1)])
            past = np.zeros((L, P), dtype=np.int64)
            for k in range(1, L + 1):
                if valid[k - 1]:
                    a = area[b - k] if b >= k else ring["areas"][L - (k - b)]
                    past[k - 1, : len(a)] = a[:P]
            tables.append(_Table(S.mask_iou_table(inter[b], np.broadcast_to(area[b], (L, P)), past), valid))
            for e in frames[b]:
                e.slot = int(labs[order[b]][e.index])
                e.support = int(area[b, e.slot])  # the mask's area in image pixels
        ring["areas"] = (ring["areas"] + [area[b].copy() for b in range(B)])[-L:]
        ring["n"] = min(L, n_hist + B)
        self._mask_ring = ring
        return tables

    def track_outputs(self, outputs, use_tables: bool = True):
        """Track a whole batch: frames in ``frame_indices`` order, the pair tables computed first (``use_tables=False``: every score pair by pair on the host, the
        same numbers).  Returns a copy of ``outputs`` with ``instance_track_ids`` (B, I) int64 and ``instance_tracking_scores`` filled for poses; for masks
        ``"track_id"`` / ``"tracking_score"`` are written into each ``pred_masks`` entry (new dicts, the inputs stay as they are)."""
        import torch

        fi = outputs.frame_indices
        B = outputs.batch_size
        order = list(np.argsort(fi.cpu().numpy(), kind="stable")) if fi is not None else list(range(B))
        fidx = (lambda b: int(fi[b])) if fi is not None else (lambda b: b)
        call0 = self.n_calls
        if outputs.pred_keypoints is None and outputs.pred_masks is not None:
            frames = []
            for k, b in enumerate(order):
                self.n_calls = call0 + k  # (entries carry the call they belong to)
                frames.append(self._entries(outputs.pred_masks[b], lazy=use_tables))
            self.n_calls = call0
            tables = self._mask_tables(outputs, order, frames) if use_tables else [None] * B
            if not use_tables:
                self._mask_ring = None
            if use_tables and (not tables or tables[0] is None):  # no device tables for this batch: the host features after all
                for fr in frames:
                    for e in fr:
                        e.support = self._feature(e).area
            new_masks: List[List[dict]] = [[] for _ in range(B)]
            for k, b in enumerate(order):
                ids, tsc = self._track_entries(frames[k], len(outputs.pred_masks[b]), fidx(b), tables[k])
                new_masks[b] = [dict(m, track_id=int(ids[j]), tracking_score=float(tsc[j])) for j, m in enumerate(outputs.pred_masks[b])]
            return replace(outputs, pred_masks=new_masks)
        kp = outputs.pred_keypoints
        if kp is None:
            raise ValueError("track_outputs needs pred_keypoints or pred_masks")
        kp = kp.detach().cpu().numpy().astype(np.float64)
        isc = outputs.instance_scores.detach().cpu().numpy() if outputs.instance_scores is not None else None
        valid = outputs.instance_valid.detach().cpu().numpy().astype(bool) if outputs.instance_valid is not None else None
        frames, rows_of = [], []
        for k, b in enumerate(order):
            rows = np.nonzero(valid[b] if valid is not None else ~np.isnan(kp[b]).all(axis=(1, 2)))[0]  # NaN-padded slots are no instances (``instance_valid`` names them when set)
            self.n_calls = call0 + k
            ents = self._entries(kp[b][rows], None if isc is None else isc[b][rows])
            frames.append(ents)
            rows_of.append(rows)
        self.n_calls = call0
        tables = self._pose_tables(frames, use_tables)
        ids_out = np.full(kp.shape[:2], -1, dtype=np.int64)
        tsc_out = np.full(kp.shape[:2], np.nan, dtype=np.float64)
        for k, b in enumerate(order):
            ids, tsc = self._track_entries(frames[k], len(rows_of[k]), fidx(b), tables[k])
            ids_out[b, rows_of[k]], tsc_out[b, rows_of[k]] = ids, tsc
        return replace(outputs, instance_track_ids=torch.from_numpy(ids_out), instance_tracking_scores=torch.from_numpy(tsc_out))
