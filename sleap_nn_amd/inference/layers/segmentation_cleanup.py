"""``CleanupSegmentationLayer``: bottom-up instance segmentation with ``mask_cleanup=True`` (sleap_nn/inference/layers/segmentation.py:102-266 with
the knob on; ``_clean_instance_mask`` at radius 0, inference/segmentation.py:240-273).

Each instance keeps its largest 4-connected component and has its interior holes filled before the area floor and the packaging of
``SegmentationLayer``; the cleanup runs on the device label map directly after the assignment and the distance gate (``ph_seg_cleanup``,
csrc/seg_cleanup_kernels.hip) and its results come down with the grouping's one host read.  For CPU tensors the same contract runs on the host
(``inference/ops/segmentation.py::clean_label_map``).  ``SegmentationLayer`` itself keeps refusing the knob; ``predictor._select_layer`` builds
this class when ``mask_cleanup`` is asked for.

Not built (each raises ``NotImplementedError`` naming the knob): ``mask_cleanup_radius > 0`` (OpenCV's elliptical open / close),
``merge_fragments`` together with ``mask_cleanup`` (``merge_fragments`` alone is ``layers/segmentation_merge.py``), ``mask_output`` other than
``"mask"``.  Tiled inference wraps this layer in ``TiledSegmentationLayer`` (``layers/tiled.py``).
"""
from __future__ import annotations

from sleap_nn_amd.inference.backends import ModelBackend
from sleap_nn_amd.inference.layers.segmentation import SegmentationLayer


class CleanupSegmentationLayer(SegmentationLayer):
    """``SegmentationLayer`` whose grouping runs with ``mask_cleanup``; every other argument as there (``mask_cleanup=False`` is accepted and gives the base behaviour)."""

    def __init__(self, backend: ModelBackend, output_stride: int, *args, mask_cleanup: bool = True, **kw) -> None:
        super().__init__(backend, output_stride, *args, mask_cleanup=False, **kw)
        self.mask_cleanup = bool(mask_cleanup)
