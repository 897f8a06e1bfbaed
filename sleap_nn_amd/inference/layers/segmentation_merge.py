"""``MergeSegmentationLayer``: bottom-up instance segmentation with ``merge_fragments=True`` (sleap_nn/inference/layers/segmentation.py:212-226;
``merge_instances``, inference/segmentation.py:424-782).

One animal split into two abutting fragments is what the offset grouping gets wrong; the merge re-fuses such fragments and keeps touching distinct
animals apart.  After the assignment and the distance gate, before the area floor and the packaging of ``SegmentationLayer``, a region-adjacency graph
over the frame's candidate masks is agglomerated: masks are neighbours when their dilations touch, an edge's affinity is
``contact_gate * (w_valley * ridge + w_offset * offset_agreement) / (w_valley + w_offset)``.  The per-pixel tables (contact counts, offset moments, ridge
minima) are computed on the device label map (``ph_seg_merge_tables``, csrc/seg_merge_kernels.hip) and come down with the grouping's one host read; the
graph (tens of nodes) is host work (``inference/ops/segmentation_merge.py``).  For CPU tensors the same contract runs on the host.
``SegmentationLayer`` itself keeps refusing the knob; ``predictor._select_layer`` builds this class when ``merge_fragments`` is asked for.

Not built (each raises ``NotImplementedError`` naming the knobs): ``merge_fragments`` together with ``mask_cleanup`` (cleaned masks overlap through their
filled holes, so the label map no longer carries membership), ``mask_cleanup_radius > 0``, ``mask_output`` other than ``"mask"``.  Tiled inference wraps
this layer in ``TiledSegmentationLayer`` (``layers/tiled.py``).
"""
from __future__ import annotations

from sleap_nn_amd.inference.backends import ModelBackend
from sleap_nn_amd.inference.layers.segmentation import SegmentationLayer
from sleap_nn_amd.inference.ops.segmentation_merge import check_merge_args


class MergeSegmentationLayer(SegmentationLayer):
    """``SegmentationLayer`` whose grouping runs with ``merge_fragments`` and the ``merge_*`` knobs (defaults as the reference); every other argument as there
    (``merge_fragments=False`` is accepted and gives the base behaviour).  ``join_bias`` is the multicut's decision boundary (0.5 in the reference's layer)."""

    def __init__(self, backend: ModelBackend, output_stride: int, *args, merge_fragments: bool = True, mask_cleanup: bool = False, join_bias: float = 0.5, **kw) -> None:
        if merge_fragments and mask_cleanup:
            raise NotImplementedError("merge_fragments=True together with mask_cleanup=True is not built on the MI355X path (cleaned masks overlap, the label "
                                      "map no longer carries membership): see inference/layers/segmentation_merge.py")
        super().__init__(backend, output_stride, *args, merge_fragments=False, mask_cleanup=mask_cleanup, **kw)
        check_merge_args(self.merge_method, self.merge_dilate, device=False)
        self.merge_fragments = bool(merge_fragments)
        self.join_bias = float(join_bias)

    def _grouping_kw(self) -> dict:
        if not self.merge_fragments:
            return {}
        return dict(merge_fragments=True, merge_method=self.merge_method, merge_thresholds=self.merge_thresholds, merge_w_valley=self.merge_w_valley,
                    merge_w_offset=self.merge_w_offset, merge_dilate=self.merge_dilate, join_bias=self.join_bias)
