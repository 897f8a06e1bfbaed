"""``TrackerConfig`` and ``apply_tracking`` (sleap_nn/inference/tracking.py:49-362) on ``Outputs`` batches.

``apply_tracking(list_of_outputs, config)`` resolves the task defaults as the reference does on the labels' content, builds one fresh ``Tracker`` and tracks
the batches in (video, frame) order with ``Tracker.track_outputs``.  ``use_flow=True`` (with ``allow_flow=True``, this project's opt-in: see ``tracker.py``) needs the
original frames, ``apply_tracking(..., frames=...)``; ``Predictor.predict`` hands them over.  The post-tracking cleanup (``tracking_clean_instance_count``,
``post_connect_single_breaks``) is not built: each raises ``NotImplementedError`` naming the knob.
"""
from __future__ import annotations

from dataclasses import dataclass, replace
from typing import List, Optional, Sequence

from sleap_nn_amd.tracking.tracker import Tracker

DEFAULT_WINDOW_SIZE = 5
DEFAULT_MASK_WINDOW_SIZE = 25


@dataclass(frozen=True, eq=False)
class TrackerConfig:
    """Every knob of the reference's frozen ``TrackerConfig``, with its defaults.  ``*_explicit=False`` lets ``apply_tracking`` substitute the task's defaults:
    ``euclidean_dist`` / ``centroids`` for a 1-node skeleton, ``mask_iou`` / ``masks`` (window 25, ``local_queues``) for mask-only outputs."""

    window_size: int = DEFAULT_WINDOW_SIZE
    min_new_track_points: int = 0
    candidates_method: str = "fixed_window"
    min_match_points: int = 0
    features: str = "keypoints"
    scoring_method: str = "oks"
    scoring_reduction: str = "mean"
    robust_best_instance: float = 1.0
    oks_stddev: Optional[float] = None
    track_matching_method: str = "hungarian"
    max_tracks: Optional[int] = None
    use_flow: bool = False
    of_img_scale: float = 1.0
    of_window_size: int = 21
    of_max_levels: int = 3
    use_kalman: bool = False
    kf_track_features: str = "centroid"
    kf_init_frame_count: int = 10
    kf_node_indices: Optional[list] = None
    kf_reset_gap_size: int = 5
    tracking_target_instance_count: Optional[int] = None
    tracking_pre_cull_to_target: int = 0
    tracking_pre_cull_iou_threshold: float = 0.0
    tracking_clean_instance_count: int = 0
    tracking_clean_iou_threshold: float = 0.0
    post_connect_single_breaks: bool = False
    scoring_method_explicit: bool = True
    features_explicit: bool = True
    candidates_method_explicit: bool = True
    allow_flow: bool = False  # OURS, not the reference's: use_flow=True is built only with it (the flow is this project's pyr_lk / ph_flow_track, not OpenCV's)


def is_mask_mode(outputs_list: Sequence) -> bool:
    """Mask-only outputs: some frame has masks and none has keypoint instances."""
    return any(o.pred_masks is not None and any(len(f) for f in o.pred_masks) for o in outputs_list) and not any(o.pred_keypoints is not None for o in outputs_list)


def resolve_config(config: TrackerConfig, n_nodes: Optional[int], mask_mode: bool) -> dict:
    """The keyword arguments of ``Tracker.from_config`` after the reference's default resolution and its refusals (``apply_tracking`` :144-252)."""
    if (config.post_connect_single_breaks or config.tracking_pre_cull_to_target) and not config.tracking_target_instance_count:
        raise ValueError("post_connect_single_breaks=True and tracking_pre_cull_to_target require tracking_target_instance_count to be set.")
    scoring, features, window, method, max_tracks = config.scoring_method, config.features, config.window_size, config.candidates_method, config.max_tracks
    if n_nodes == 1:
        if not config.scoring_method_explicit:
            scoring = "euclidean_dist"
        if not config.features_explicit:
            features = "centroids"
    if mask_mode:
        if not config.scoring_method_explicit:
            scoring = "mask_iou"
        if not config.features_explicit:
            features = "masks"
        if features != "masks" or scoring != "mask_iou":
            raise ValueError("Tracking a bottom-up segmentation (mask-only) model requires features='masks' and scoring_method='mask_iou' "
                             f"(got features={features!r}, scoring_method={scoring!r}). Leave features / scoring_method unset to auto-select them.")
        if config.use_flow or config.use_kalman:
            raise ValueError("Mask tracking does not support motion models (use_flow / use_kalman); they are out of scope for the segmentation tracker.")
        if config.tracking_pre_cull_to_target or config.tracking_clean_instance_count or config.post_connect_single_breaks:
            raise ValueError("Mask tracking does not support the instance cull/clean/connect options (tracking_pre_cull_to_target / "
                             "tracking_clean_instance_count / post_connect_single_breaks); these operate on keypoint poses, not masks.")
        if config.window_size == DEFAULT_WINDOW_SIZE:
            window = DEFAULT_MASK_WINDOW_SIZE
        if not config.candidates_method_explicit:
            method = "local_queues"
        if max_tracks is None and config.tracking_target_instance_count:
            max_tracks = config.tracking_target_instance_count
    if config.tracking_clean_instance_count:
        raise NotImplementedError("tracking_clean_instance_count is not built on the MI355X path (the post-tracking cull and connect of inference/tracking.py): "
                                  "see sleap_nn_amd/tracking/config.py")
    if config.post_connect_single_breaks:
        raise NotImplementedError("post_connect_single_breaks is not built on the MI355X path (the post-tracking cleanup of inference/tracking.py): "
                                  "see sleap_nn_amd/tracking/config.py")
    return dict(window_size=window, min_new_track_points=config.min_new_track_points, candidates_method=method, min_match_points=config.min_match_points,
                features=features, scoring_method=scoring, scoring_reduction=config.scoring_reduction, robust_best_instance=config.robust_best_instance,
                oks_stddev=config.oks_stddev, track_matching_method=config.track_matching_method, max_tracks=max_tracks, use_flow=config.use_flow,
                of_img_scale=config.of_img_scale, of_window_size=config.of_window_size, of_max_levels=config.of_max_levels, use_kalman=config.use_kalman,
                kf_track_features=config.kf_track_features, kf_init_frame_count=config.kf_init_frame_count, kf_node_indices=config.kf_node_indices,
                kf_reset_gap_size=config.kf_reset_gap_size, tracking_target_instance_count=config.tracking_target_instance_count,
                tracking_pre_cull_to_target=config.tracking_pre_cull_to_target, tracking_pre_cull_iou_threshold=config.tracking_pre_cull_iou_threshold,
                allow_flow=config.allow_flow)


def build_tracker(config: TrackerConfig, outputs_list: Sequence) -> Tracker:
    kp = next((o.pred_keypoints for o in outputs_list if o.pred_keypoints is not None), None)
    return Tracker.from_config(**resolve_config(config, None if kp is None else int(kp.shape[2]), is_mask_mode(outputs_list)))


def apply_tracking(outputs_list: Sequence, config: TrackerConfig, use_tables: bool = True, frames=None) -> List:
    """Track every frame of ``outputs_list`` (one ``Outputs`` per batch) with a fresh ``Tracker``: batches in (video, first frame) order, frames inside a batch
    in ``frame_indices`` order.  Returns the tracked ``Outputs`` in the order given; they share one ``track_objects`` dict, so that ``to_instances`` /
    ``to_labels`` hand out ONE ``sio.Track`` per id across the batches.  ``frames``: with ``use_flow`` the ORIGINAL frames of the whole call, ``(N, H, W)``,
    ``(N, H, W, 1)`` or ``(N, 1, H, W)``, indexed by each batch's ``frame_indices`` (host or device; a batch's frames are uploaded once)."""
    outputs_list = list(outputs_list)
    tracker = build_tracker(config, outputs_list)
    if tracker.use_flow and frames is None:
        raise ValueError("use_flow=True needs the frames: apply_tracking(outputs, config, frames=...)")

    def images_of(o):
        if not tracker.use_flow:
            return None
        if o.frame_indices is None:
            if len(outputs_list) != 1:
                raise ValueError("use_flow: Outputs.frame_indices is needed to find a batch's frames")
            return frames
        return [frames[int(i)] for i in o.frame_indices]

    def key(i):
        o = outputs_list[i]
        v = int(o.video_indices.min()) if o.video_indices is not None and o.video_indices.numel() else 0
        f = int(o.frame_indices.min()) if o.frame_indices is not None and o.frame_indices.numel() else i
        return (v, f, i)

    shared: dict = {}
    out: List = [None] * len(outputs_list)
    for i in sorted(range(len(outputs_list)), key=key):
        out[i] = replace(tracker.track_outputs(outputs_list[i], images=images_of(outputs_list[i]), use_tables=use_tables), track_objects=shared)
    return out
