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

``use_flow`` (the reference's ``FlowShiftTracker``, ``from_config(use_flow=True, allow_flow=True)``): a candidate's feature is the feature of the past instance's
keypoints MOVED onto the current frame by pyramidal Lucas-Kanade flow between the two ORIGINAL frames (``image=`` / ``images=``; lost nodes NaN); the support test
stays on the source instance, and every instance of a queued frame is a candidate of its id (not only the first).  The flow is ``flow.pyr_lk`` -- OURS, a stand-in for
``cv2.calcOpticalFlowPyrLK`` that has not been compared with OpenCV, hence the opt-in -- on the host, ``ph_flow_pyramid`` / ``ph_flow_track`` (csrc/flow_kernels.hip) on
the device; a frame's pyramid is built once, not once per pair as in the reference.  The shifted points depend on no assignment, so with the fixed window
``track_outputs`` computes ALL (frame, lag <= min(window_size, 32), instance) flows of a batch in ONE launch, against the batch itself and the retained frames of the
last calls, and scores them with ``ph_track_pose_scores_shifted``; ``local_queues`` (a candidate can be arbitrarily old: each queue entry holds its frame's pyramid,
alive as long as the entry), ``track()`` and a window beyond 32 take one launch per frame with one job per distinct reference frame.  Without a GPU and with host
frames the same code runs ``pyr_lk``.  DESIGN.md section 4.2g.

Refused (``NotImplementedError`` naming the knob): ``use_flow`` without ``allow_flow``, ``of_img_scale != 1`` (``cv2.resize``), frames with more than one channel
(``cv2.cvtColor``), ``use_kalman`` (pykalman's EM), ``features="image"``.
"""
from __future__ import annotations

import warnings
from collections import defaultdict, deque
from dataclasses import replace
from typing import Any, Dict, List, Optional, Sequence, Tuple

import numpy as np

from sleap_nn_amd.tracking import flow as F
from sleap_nn_amd.tracking import scoring as S

_FEATURES = {"keypoints": S.keypoints_feature, "centroids": S.centroid_feature, "bboxes": S.bbox_feature, "masks": S.mask_feature}
_SCORES = ("oks", "iou", "mask_iou", "cosine_sim", "euclidean_dist")
_REDUCTIONS = ("mean", "max", "robust_quantile")
_MATCHING = ("hungarian", "greedy")
SAME_POSE_TOLERANCE = 5.0


class _Entry:
    """One instance of one call: ``src`` (keypoints or the mask entry), its feature, its support (non-NaN nodes, or mask area in image pixels), where the pair
    tables hold it (``call``, ``slot``), its row in the caller's input (``index``) and its detection score (the pre-cull sorts by it)."""

    __slots__ = ("src", "feature", "support", "call", "slot", "index", "score", "track_id", "tracking_score", "image", "frame_idx")

    def __init__(self, src, feature, support, call, slot, index, score, image=None, frame_idx=None):
        self.src, self.feature, self.support, self.call, self.slot, self.index, self.score = src, feature, support, call, slot, index, score
        self.track_id: Optional[int] = None
        self.tracking_score: Optional[float] = None
        self.image, self.frame_idx = image, frame_idx  # the flow tracker: the instance's frame (a ``_FlowFrame``, kept alive by this reference) and its index

    def again(self) -> "_Entry":
        return _Entry(self.src, self.feature, self.support, self.call, self.slot, self.index, self.score, self.image, self.frame_idx)


class _FlowFrame:
    """A frame as the flow reads it: the uint8 image on the host with its pyramid (built on first use), or the device pyramid (``levels``, level 0 first)."""

    __slots__ = ("host", "levels", "_pyramid")

    def __init__(self, host=None, levels=None):
        self.host, self.levels, self._pyramid = host, levels, None

    def pyramid(self, win: int, max_level: int):
        if self._pyramid is None:
            self._pyramid = F.build_pyramid(self.host, win, max_level)
        return self._pyramid


class _FlowScores:
    """Scores of one frame's instances against flow-shifted candidates the batch table does not hold: ``rows[id(past)][cur.slot]``."""

    def __init__(self):
        self.rows: Dict[int, np.ndarray] = {}

    def lookup(self, cur: _Entry, past: _Entry) -> float:
        return float(self.rows[id(past)][cur.slot])


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

    def flow_candidates(self) -> Dict[Any, List[_Entry]]:
        """The flow tracker's candidates per track id (tracker.py:770-805): EVERY instance of every queued frame under its id, not only the first of a frame."""
        out: Dict[Any, List[_Entry]] = defaultdict(list)
        for fr in self.tracker_queue:
            for i, e in enumerate(fr.entries):
                out[fr.track_ids[i]].append(e)
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

    def flow_candidates(self) -> Dict[Any, List[_Entry]]:
        """The flow tracker's candidates per track id in the reference's order (tracker.py:731-768): the queues' instances grouped by frame index, groups in
        the order the queues name them, each instance under its track id."""
        groups: Dict[Any, List[_Entry]] = {}
        for _tid, q in self.tracker_queue.items():
            for e in q:
                groups.setdefault(e.frame_idx, []).append(e)
        out: Dict[Any, List[_Entry]] = defaultdict(list)
        for lst in groups.values():
            for e in lst:
                out[e.track_id].append(e)
        return out

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
                 tracking_target_instance_count: Optional[int] = None, tracking_pre_cull_to_target: int = 0, tracking_pre_cull_iou_threshold: float = 0,
                 use_flow: bool = False, of_window_size: int = 21, of_max_levels: int = 3) -> None:
        self.candidate = candidate
        self.min_match_points = min_match_points
        self.features, self.scoring_method, self.scoring_reduction = features, scoring_method, scoring_reduction
        self.track_matching_method, self.robust_best_instance, self.oks_stddev = track_matching_method, robust_best_instance, oks_stddev
        self.is_local_queue = is_local_queue
        self.tracking_target_instance_count = tracking_target_instance_count
        self.tracking_pre_cull_to_target = tracking_pre_cull_to_target
        self.tracking_pre_cull_iou_threshold = tracking_pre_cull_iou_threshold
        self.use_flow, self.of_window_size, self.of_max_levels = bool(use_flow), int(of_window_size), int(of_max_levels)
        self.flow_device: Optional[bool] = None  # where the flow runs: None = the device when the frames are there or a GPU is present, False = pyr_lk on the host
        self.flow_launches = 0  # ph_flow_track launches / pyr_lk calls so far
        self.flow_cpu_calls = 0
        self._flow_ring: Optional[deque] = None  # (frame, points (I, N, 2) float32) of the last calls, newest last: what the batch's flow jobs reach back to
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
                    tracking_pre_cull_iou_threshold: float = 0, allow_flow: bool = False) -> "Tracker":
        """The reference's signature and defaults (tracker.py:128-158).  ``max_tracks`` with ``fixed_window`` switches to ``local_queues`` (the only maker that
        honours the cap); ``oks_stddev=None`` resolves to 0.025.  ``allow_flow`` is OURS, not the reference's: ``use_flow=True`` builds the flow-shift tracker only
        with it, because its optical flow is this project's ``pyr_lk`` / ``ph_flow_track`` and has not been compared with OpenCV's numbers."""
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
        if use_flow and not allow_flow:
            raise NotImplementedError("use_flow=True runs this project's own pyramidal Lucas-Kanade flow (sleap_nn_amd/tracking/flow.py), which has not been compared "
                                      "with OpenCV's: pass allow_flow=True to use it; see sleap_nn_amd/tracking/tracker.py")
        if use_flow:
            if of_img_scale != 1:
                raise NotImplementedError("of_img_scale != 1 is not built on the MI355X path (cv2.resize of the frames): see sleap_nn_amd/tracking/tracker.py")
            if features == "masks" or scoring_method == "mask_iou":
                raise ValueError("use_flow moves keypoints: features='masks' / scoring_method='mask_iou' cannot be combined with it")
            if not (F.MIN_WIN <= int(of_window_size) <= F.MAX_WIN) or not (0 <= int(of_max_levels) < F.MAX_LEVELS):
                raise ValueError(f"of_window_size must lie in [{F.MIN_WIN}, {F.MAX_WIN}] and of_max_levels in [0, {F.MAX_LEVELS - 1}], got {of_window_size} and {of_max_levels}")
        if use_kalman:
            raise NotImplementedError("use_kalman=True is not built on the MI355X path (pykalman's EM fit): see sleap_nn_amd/tracking/tracker.py")
        if features == "image":
            raise NotImplementedError("features='image' is not built on the MI355X path: see sleap_nn_amd/tracking/tracker.py")
        if oks_stddev is None:
            oks_stddev = 0.025
        return cls(candidate=candidate, min_match_points=min_match_points, features=features, scoring_method=scoring_method, scoring_reduction=scoring_reduction,
                   robust_best_instance=robust_best_instance, oks_stddev=oks_stddev, track_matching_method=track_matching_method, is_local_queue=local,
                   tracking_target_instance_count=tracking_target_instance_count, tracking_pre_cull_to_target=tracking_pre_cull_to_target,
                   tracking_pre_cull_iou_threshold=tracking_pre_cull_iou_threshold, use_flow=use_flow, of_window_size=of_window_size, of_max_levels=of_max_levels)

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

    @staticmethod
    def _in_table(call: int, slot: int, past: _Entry, table: Optional[_Table]) -> bool:
        if table is None:
            return False
        k = call - past.call
        return bool(1 <= k <= len(table.valid) and table.valid[k - 1] and slot >= 0 and past.slot >= 0)

    def _score(self, cur: _Entry, past: _Entry, table: Optional[_Table], shifted: Optional[_FlowScores] = None) -> float:
        if self._in_table(cur.call, cur.slot, past, table):
            self.table_hits += 1
            return float(table.scores[cur.call - past.call - 1, cur.slot, past.slot])
        self.pair_calls += 1
        if self.use_flow:  # (the candidate's feature is its SHIFTED pose: never the pair function on the past instance itself)
            return shifted.lookup(cur, past)
        return self.pair_score(self._feature(cur), self._feature(past))

    # -- optical flow (tracker.py:680-807) --------------------------------------------------------------------------
    def _flow_frames(self, images, n: int) -> List[_FlowFrame]:
        """``n`` frames (a tensor / array with a leading frame axis, or a list of frames) as ``_FlowFrame``s: gray uint8, on the device -- uploaded in one copy,
        the pyramids of all in one ``ph_flow_pyramid`` call -- when the frames are device tensors or a GPU is present, on the host otherwise."""
        import torch

        if images is None:
            raise ValueError("use_flow=True needs the frames: pass image= to track() / images= to track_outputs() (the ORIGINAL frames, the space of the keypoints)")
        if len(images) != n:
            raise ValueError(f"use_flow: {len(images)} frames for {n} calls")
        if n == 0:
            return []
        grays = [F.as_gray_u8(im) for im in images]
        batch = torch.stack(grays)
        if (batch.is_cuda or torch.cuda.is_available()) if self.flow_device is None else self.flow_device:
            batch = batch.cuda() if not batch.is_cuda else batch
            return [_FlowFrame(levels=lv) for lv in F.pyramid_device(batch, self.of_window_size, self.of_max_levels)]
        host = batch.cpu().numpy()
        return [_FlowFrame(host=host[i]) for i in range(n)]

    def _run_flow(self, jobs: List[Tuple[_FlowFrame, _FlowFrame, np.ndarray]]) -> List[np.ndarray]:
        """``(reference frame, current frame, points (P, 2) float32)`` per job -> the shifted points per job, float32 with NaN for lost points.  All jobs of a
        call are ONE ``ph_flow_track`` launch on the device; on the host one ``pyr_lk`` per job, the pyramids built once per frame."""
        if not jobs:
            return []
        win, lv = self.of_window_size, self.of_max_levels
        if jobs[0][1].levels is not None:
            self.flow_launches += 1
            return [s for s, _st in F.track_device([(r.levels, c.levels, p) for r, c, p in jobs], win, lv)]
        out = []
        for r, c, p in jobs:
            self.flow_cpu_calls += 1
            out.append(F.pyr_lk(None, None, p, win, lv, ref_pyramid=r.pyramid(win, lv), new_pyramid=c.pyramid(win, lv))[0])
        return out

    def _native_block(self, feats: list) -> Optional[np.ndarray]:
        """Features as ``(n, D / 2, 2)`` float64 for the native pair scores; None for shapes the NumPy functions refuse (they are left to refuse them)."""
        if self.scoring_method not in S.METHODS or not feats:
            return None
        first = np.asarray(feats[0])
        D = first.size
        if D == 0 or D % 2 or (self.scoring_method == "iou" and D != 4) or (self.scoring_method == "cosine_sim" and first.ndim != 1):
            return None
        return np.stack([np.asarray(f, dtype=np.float64).reshape(D // 2, 2) for f in feats])

    def _shifted_scores(self, cur_feats: list, groups: List[list]) -> List[np.ndarray]:
        """Scores of one frame's features against groups of shifted candidate features: per group ``(len(cur_feats), len(group))``, ``ph_track_pose_scores_shifted``
        in chunks of 32 groups."""
        cur = self._native_block(cur_feats)
        blocks = [self._native_block(g) for g in groups]
        if cur is None or any(b is None or b.shape[1:] != cur.shape[1:] for b in blocks):
            return [np.array([[self.pair_score(a, p) for p in g] for a in cur_feats], dtype=np.float64).reshape(len(cur_feats), len(g)) for g in groups]
        I = max(len(cur), max(len(b) for b in blocks))
        cur_t = np.full((1, I) + cur.shape[1:], np.nan)
        cur_t[0, : len(cur)] = cur
        out = []
        for s in range(0, len(blocks), S.MAX_TABLE_LAGS):
            part = blocks[s : s + S.MAX_TABLE_LAGS]
            hist = np.full((1, len(part), I) + cur.shape[1:], np.nan)
            for g, b in enumerate(part):
                hist[0, g, : len(b)] = b
            sc = S.pose_pair_scores_shifted(cur_t, hist, np.array([len(cur)], np.int32), np.array([[len(b) for b in part]], np.int32), self.scoring_method, self.oks_stddev)
            out.extend(sc[0, g, : len(cur), : len(b)] for g, b in enumerate(part))
        return out

    def _flow_scores(self, cur_entries: List[_Entry], pasts: List[_Entry], image: _FlowFrame) -> Optional[_FlowScores]:
        """One frame against the candidates ``pasts`` no batch table holds: the candidates grouped by their frame (``local_queues``: by frame index, the first
        one's image, as the reference groups them), one flow job per distinct frame in one launch, the feature function on the shifted points, native scores."""
        if not pasts or not cur_entries:
            return None
        groups: Dict[Any, List[_Entry]] = {}
        for p in pasts:
            groups.setdefault(p.frame_idx if self.is_local_queue else id(p.image), []).append(p)
        lists = list(groups.values())
        jobs = [(g[0].image, image, np.concatenate([np.asarray(p.src, dtype=np.float32) for p in g]).reshape(-1, 2)) for g in lists]
        fn = _FEATURES[self.features]
        feats = []
        for g, sh in zip(lists, self._run_flow(jobs)):
            n_nodes = len(g[0].src)
            feats.append([fn(sh[i * n_nodes : (i + 1) * n_nodes]) for i in range(len(g))])
        by_slot = sorted(cur_entries, key=lambda e: e.slot)
        assert [e.slot for e in by_slot] == list(range(len(by_slot)))
        res = _FlowScores()
        for g, sc in zip(lists, self._shifted_scores([e.feature for e in by_slot], feats)):
            for j, p in enumerate(g):
                res.rows[id(p)] = sc[:, j]
        return res

    def _flow_tables(self, frames: List[List[_Entry]], images: List[_FlowFrame], use_native: bool) -> List[Optional[_Table]]:
        """The fixed window's batch: the flows of EVERY (frame b, lag k <= L, instance of the frame k calls earlier) -- the batch against itself and the retained
        frames of the last L calls -- as ONE ``ph_flow_track`` launch before the frame-by-frame matching starts (a shifted point depends on no assignment), the
        feature function on the shifted points, ``ph_track_pose_scores_shifted``.  Flows of instances that end up outside the queue are computed and ignored."""
        B, L = len(frames), self.table_lags
        ok = use_native and not self.is_local_queue and self.candidate.window_size <= S.MAX_TABLE_LAGS and self.scoring_method in S.METHODS and any(frames)
        ring = self._flow_ring if self._flow_ring is not None and self._flow_ring.maxlen == L else deque(maxlen=L)
        if ok:
            n_nodes = {len(e.src) for fr in frames for e in fr} | {pts.shape[1] for _im, pts in ring if len(pts)}
            ok = len(n_nodes) == 1
        if not ok:
            self._flow_ring = None
            return [None] * B
        N = n_nodes.pop()
        pts_of = [np.stack([np.asarray(e.src, dtype=np.float32) for e in fr]) if fr else np.zeros((0, N, 2), np.float32) for fr in frames]
        for fr in frames:
            for s, e in enumerate(fr):
                e.slot = s
        past_of = lambda b, k: (images[b - k], pts_of[b - k]) if b >= k else (ring[len(ring) - (k - b)] if k - b <= len(ring) else None)
        jobs, where = [], []
        for b in range(B):
            for k in range(1, L + 1):
                past = past_of(b, k)
                if past is not None and len(past[1]) and frames[b]:
                    jobs.append((past[0], images[b], past[1].reshape(-1, 2)))
                    where.append((b, k))
        fn = _FEATURES[self.features]
        cur_feats = [[e.feature for e in fr] for fr in frames]
        probe = self._native_block([f for fr in cur_feats for f in fr])
        if probe is None:
            self._flow_ring = None
            return [None] * B
        I = max(max(len(fr) for fr in frames), max([len(pts) for _im, pts in ring], default=0))
        cur = np.full((B, I) + probe.shape[1:], np.nan)
        hist = np.full((B, L, I) + probe.shape[1:], np.nan)
        counts_hist = np.zeros((B, L), np.int32)
        for b, fr in enumerate(cur_feats):
            if fr:
                cur[b, : len(fr)] = self._native_block(fr)
        for (b, k), sh in zip(where, self._run_flow(jobs)):
            sh = sh.reshape(-1, N, 2)
            hist[b, k - 1, : len(sh)] = self._native_block([fn(p) for p in sh])
            counts_hist[b, k - 1] = len(sh)
        sc = S.pose_pair_scores_shifted(cur, hist, np.array([len(fr) for fr in frames], np.int32), counts_hist, self.scoring_method, self.oks_stddev)
        tables = [_Table(sc[b], np.array([past_of(b, k) is not None for k in range(1, L + 1)])) for b in range(B)]
        for b in range(B):
            ring.append((images[b], pts_of[b]))
        self._flow_ring = ring
        return tables

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

    def _track_entries(self, entries: List[_Entry], n: int, frame_idx, table: Optional[_Table] = None, image: Optional[_FlowFrame] = None) -> Tuple[np.ndarray, np.ndarray]:
        masks = bool(entries) and isinstance(entries[0].src, dict)
        all_entries = entries
        if self.use_flow:
            if masks:
                raise ValueError("use_flow moves keypoints: it cannot track segmentation masks")
            for e in entries:
                e.image, e.frame_idx = image, frame_idx
        if not masks and self.tracking_target_instance_count and self.tracking_pre_cull_to_target:
            entries = cull_frame_instances(entries, self.tracking_target_instance_count, self.tracking_pre_cull_iou_threshold)
        cand = self.candidate
        cur = cand.make(entries, frame_idx)
        self.last_scores = None
        if cand.tracker_queue:
            tracks = cand.current_tracks
            shifted = None
            if self.use_flow:  # the candidates moved onto this frame; the support test stays on the SOURCE instance
                moved = cand.flow_candidates()
                past = {t: moved.get(t, []) for t in tracks}
                slot = all_entries[0].slot if all_entries else -1
                shifted = self._flow_scores(all_entries, [p for t in tracks for p in past[t] if not self._in_table(self.n_calls, slot, p, table)], image)
            else:
                past = {t: cand.candidates_of(t) for t in tracks}
            scores = np.zeros((len(entries), len(tracks)))
            for i, e in enumerate(entries):
                for j, t in enumerate(tracks):
                    scores[i][j] = self._reduce([self._score(e, p, table, shifted) for p in past[t] if p.support > self.min_match_points])
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

    def track(self, instances, frame_idx, instance_scores=None, image=None) -> Tuple[np.ndarray, np.ndarray]:
        """One frame, every score in NumPy.  ``instances``: ``(I, N, 2)`` keypoints (NaN = missing) or a list of ``pred_masks`` entries; ``instance_scores``
        ``(I,)``: the detection scores the pre-cull sorts by (a mask entry's ``"score"`` by default).  ``image``: the ORIGINAL frame (the reference's ``lf.image``,
        the space of the keypoints), needed with ``use_flow`` and ignored without: ``(H, W)``, ``(H, W, 1)`` or ``(1, H, W)``, uint8 or float, host or device; the
        flows of the frame are one launch with one job per queued frame, scored by ``ph_track_pose_scores_shifted``."""
        handle = self._flow_frames([image] if image is not None else None, 1)[0] if self.use_flow else None
        ids, tsc = self._track_entries(self._entries(instances, instance_scores), len(instances), frame_idx, image=handle)
        self._pose_hist, self._pose_n_hist, self._mask_ring, self._flow_ring = None, 0, None, None  # the tables' history does not hold this call: start it again
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

    def track_outputs(self, outputs, images=None, use_tables: bool = True):
        """Track a whole batch: frames in ``frame_indices`` order, the pair tables computed first (``use_tables=False``: every score pair by pair on the host, the
        same numbers).  Returns a copy of ``outputs`` with ``instance_track_ids`` (B, I) int64 and ``instance_tracking_scores`` filled for poses; for masks
        ``"track_id"`` / ``"tracking_score"`` are written into each ``pred_masks`` entry (new dicts, the inputs stay as they are).  ``images``: with ``use_flow`` the
        batch's ORIGINAL frames, ``(B, H, W)``, ``(B, H, W, 1)`` or ``(B, 1, H, W)``, in the order of the batch (see ``track``); host frames are uploaded once."""
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
        handles: List[Optional[_FlowFrame]] = [None] * B
        if self.use_flow:
            if images is not None and len(images) != B:
                raise ValueError(f"use_flow: {len(images)} frames for a batch of {B}")
            handles = self._flow_frames(None if images is None else [images[b] for b in order], B)
            tables = self._flow_tables(frames, handles, use_tables)
        else:
            tables = self._pose_tables(frames, use_tables)
        ids_out = np.full(kp.shape[:2], -1, dtype=np.int64)
        tsc_out = np.full(kp.shape[:2], np.nan, dtype=np.float64)
        for k, b in enumerate(order):
            ids, tsc = self._track_entries(frames[k], len(rows_of[k]), fidx(b), tables[k], handles[k])
            ids_out[b, rows_of[k]], tsc_out[b, rows_of[k]] = ids, tsc
        return replace(outputs, instance_track_ids=torch.from_numpy(ids_out), instance_tracking_scores=torch.from_numpy(tsc_out))
