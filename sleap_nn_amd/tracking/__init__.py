"""Cross-frame tracking (sleap_nn/tracking/, sleap_nn/inference/tracking.py): ``Tracker``, ``TrackerConfig``, ``apply_tracking``."""
from sleap_nn_amd.tracking.config import TrackerConfig, apply_tracking, build_tracker, resolve_config
from sleap_nn_amd.tracking.tracker import FixedWindowCandidates, LocalQueueCandidates, Tracker

__all__ = ["Tracker", "TrackerConfig", "apply_tracking", "build_tracker", "resolve_config", "FixedWindowCandidates", "LocalQueueCandidates"]
