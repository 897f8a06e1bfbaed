"""Top-down instance segmentation without a GPU: the mask layer, the crop geometry and the host placement against the reference's recorded results
(tests/golden/topdown_segmentation.npz, tools/gen_topdown_seg_golden.py), the run directories' layer selection, what stays refused, and the ``Outputs``
helpers.  The resample rule of ``decode/`` is the generator's stand-in for sleap-io's (``F.interpolate(mode="nearest")``); the rounding, pad and clip are
the reference's ``decode_mask_to_image_res``."""
import json
import os

import numpy as np
import pytest
import torch

from tests import _golden as G
from tests.test_segmentation_cpu import StubBackend

TDS = G.load("topdown_segmentation.npz")
PARAMS = json.loads(str(TDS["layer/params"]))
CASES = ("plain", "sized")
CENTROID_DIR = os.path.join(G.GOLDEN_DIR, "ckpt_dirs", "tiny_centroid_seg")
SEG_DIR = os.path.join(G.GOLDEN_DIR, "ckpt_dirs", "tiny_centered_instance_segmentation")
FRAME_HW = tuple(TDS["layer/frames"].shape[-2:])


def recorded_entries(case):
    """The reference's entries of a case, frame by frame: ``[[{"mask", "score", "scale", "offset"}, ...], ...]`` and their flat decode list."""
    n = TDS[f"layer/{case}/n"]
    masks, scores, scales, offsets = (TDS[f"layer/{case}/{k}"] for k in ("masks", "scores", "scales", "offsets"))
    frames, k = [], 0
    for b in range(len(n)):
        frames.append([{"mask": masks[j], "score": float(scores[j]), "scale": tuple(scales[j]), "offset": tuple(offsets[j])} for j in range(k, k + int(n[b]))])
        k += int(n[b])
    return frames, [TDS[f"decode/{case}/{j}"] for j in range(k)]


def clip_to_frame(dec):
    """``decode_mask_to_image_res``' array cropped / zero-padded to the frame (what a consumer that indexes the frame does with it)."""
    out = np.zeros(FRAME_HW, dtype=bool)
    h, w = min(FRAME_HW[0], dec.shape[0]), min(FRAME_HW[1], dec.shape[1])
    out[:h, :w] = dec[:h, :w]
    return out


def test_golden_covers_the_required_cases():
    for case in CASES:
        n = TDS[f"layer/{case}/n"].tolist()
        assert n[0] in (3, 4) and n[1] in (3, 4) and n[2] == 0  # the blob-free frame
        offs, masks, scales = TDS[f"layer/{case}/offsets"], TDS[f"layer/{case}/masks"], TDS[f"layer/{case}/scales"]
        ext = np.round(masks.shape[1] / scales[:, 1]), np.round(masks.shape[2] / scales[:, 0])
        assert ((offs[:, 0] < -0.5) & (offs[:, 1] < -0.5)).any()  # a crop that spills over the left and top edge
        assert ((np.round(offs[:, 0]) + ext[1] > FRAME_HW[1]) & (np.round(offs[:, 1]) + ext[0] > FRAME_HW[0])).any()  # ... and the right and bottom edge
        assert TDS[f"layer/{case}/uncertain"].reshape(len(masks), -1).mean(1).max() <= 0.005
    assert float(TDS["layer/sized/eff"].max()) < 1.0 and not float(TDS["layer/sized/scales"][0, 0] * 2).is_integer()


def test_mask_layer_postprocess_reproduces_reference():
    from sleap_nn_amd.inference.layers import CenteredInstanceMaskLayer

    layer = CenteredInstanceMaskLayer(StubBackend(), 2)
    assert (layer.output_stride, layer.max_stride, layer.fg_threshold, layer.use_gt_peaks) == (2, 1, 0.5, False)
    out = layer.postprocess({"SegmentationHead": torch.from_numpy(TDS["mask_layer/probs"])}, None)
    assert out.crops.dtype == torch.uint8 and tuple(out.crops.shape) == TDS["mask_layer/masks"].shape and tuple(out.instance_scores.shape) == (5, 1)
    assert np.array_equal(out.crops.numpy() != 0, TDS["mask_layer/masks"])
    assert np.abs(out.instance_scores.numpy().astype(np.float64) - TDS["mask_layer/scores"]).max() <= 1e-6
    assert out.instance_scores[1, 0] == 0.0 and not out.crops[1].any()  # the empty mask scores 0


@pytest.mark.parametrize("case", CASES)
def test_host_placement_equals_reference_decode(case):
    from sleap_nn_amd.inference.ops.segmentation import mask_extent, place_crop_masks, stack_pred_masks

    frames, decoded = recorded_entries(case)
    flat = [d for f in frames for d in f]
    masks = np.stack([d["mask"] for d in flat])
    origins = np.array([[round(d["offset"][0]), round(d["offset"][1])] for d in flat])
    extents = np.array([mask_extent(d["mask"].shape, d["scale"]) for d in flat])
    out = place_crop_masks(masks, np.arange(len(flat)), origins, extents, FRAME_HW, 1)
    assert out.shape == (len(flat), 1) + FRAME_HW and out.dtype == np.uint8
    for k, dec in enumerate(decoded):
        assert np.array_equal(out[k, 0] != 0, clip_to_frame(dec)), (case, k)
        # and on a frame large enough to hold the whole decoded array: nothing but the reference's pad and drop
        big = place_crop_masks(masks[k : k + 1], np.zeros(1, np.int64), origins[k : k + 1], extents[k : k + 1], (200, 200), 1)[0, 0]
        assert np.array_equal(big[: dec.shape[0], : dec.shape[1]] != 0, dec) and int(big.sum()) == int(dec.sum())
    stack, counts = stack_pred_masks(frames, FRAME_HW)
    assert counts.tolist() == [len(f) for f in frames] and stack.shape == (3, max(counts),) + FRAME_HW and not stack[2].any()
    k = 0
    for b, f in enumerate(frames):
        for j in range(len(f)):
            assert np.array_equal(stack[b, j] != 0, clip_to_frame(decoded[k]))
            k += 1


@pytest.mark.parametrize("case", CASES)
def test_crop_mask_geometry_reproduces_recorded_floats(case):
    from sleap_nn_amd.inference.ops.segmentation import crop_mask_geometry

    masks = TDS[f"layer/{case}/masks"]
    eff = TDS[f"layer/{case}/eff"][TDS[f"layer/{case}/samples"]]
    geo = crop_mask_geometry(TDS[f"layer/{case}/topleft_sized"], eff, 1.0, PARAMS["stride"], (PARAMS["crop"], PARAMS["crop"]), masks.shape[1:])
    assert np.array_equal(geo.offset, TDS[f"layer/{case}/offsets"]) and np.array_equal(geo.scale, TDS[f"layer/{case}/scales"])  # exactly: the same host arithmetic
    assert np.array_equal(geo.origin, np.round(TDS[f"layer/{case}/offsets"]).astype(np.int32))  # (no recorded offset ends in .5)
    want = 32 if case == "plain" else 43  # 16 / (0.75 / 2) = 42.67
    assert geo.extent.tolist() == [[want, want]] * len(masks)


def test_placement_contract_on_a_hand_case():
    from sleap_nn_amd.inference.ops.segmentation import place_crop_masks

    m = np.arange(1, 7, dtype=np.uint8).reshape(1, 2, 3)
    out = place_crop_masks(m, np.array([-1, 0]), np.array([[-1, 1]]), np.array([[4, 5]]), (4, 6), 2)  # rows (v * 2) // 4, columns (u * 3) // 5
    assert not out[0, 0].any()  # the empty slot
    want = np.zeros((4, 6), np.uint8)
    rows, cols = [0, 0, 1, 1], [0, 0, 1, 1, 2]
    for y in range(4):
        for x in range(6):
            v, u = y - 1, x + 1
            if 0 <= v < 4 and 0 <= u < 5:
                want[y, x] = m[0, rows[v], cols[u]]
    assert np.array_equal(out[0, 1], want)
    t = place_crop_masks(torch.from_numpy(m), torch.tensor([-1, 0]), torch.tensor([[-1, 1]]), torch.tensor([[4, 5]]), (4, 6), 2)
    assert torch.is_tensor(t) and np.array_equal(t.numpy(), out)


def test_run_directory_pair_resolves_to_layer(monkeypatch):
    from sleap_nn_amd.inference import predictor as P
    from sleap_nn_amd.inference.layers import CenteredInstanceMaskLayer, CentroidLayer, PostprocessConfig, TopDownSegmentationLayer
    from sleap_nn_amd.inference.loaders import MODEL_TYPES, load_model_assets

    assert "centered_instance_segmentation" in MODEL_TYPES
    c, s = load_model_assets(CENTROID_DIR), load_model_assets(SEG_DIR)
    assert c.model_type == "centroid" and s.model_type == "centered_instance_segmentation"  # the real name, whatever program the network is built with
    assert s.head_config["segmentation"]["crop_size"] == 32 and s.head_config["segmentation"]["anchor_part"] is None
    monkeypatch.setattr(P, "HipBackend", lambda model, device: StubBackend(model))
    for assets in ([c, s], [s, c]):  # (before the plain centroid branch, in either order)
        layer = P._select_layer(assets, "cuda:0", PostprocessConfig(peak_threshold=0.2), 4, seg_kw={"fg_threshold": 0.4})
        assert type(layer) is TopDownSegmentationLayer and type(layer.centroid_layer) is CentroidLayer and type(layer.centered_instance_layer) is CenteredInstanceMaskLayer
        il = layer.centered_instance_layer
        assert layer.crop_size == (32, 32) and layer.place_masks is False and layer.return_crops is False and layer.mask_output == "mask" and layer.polygon_epsilon == 0.01
        assert (il.output_stride, il.max_stride, il.fg_threshold) == (2, 8, 0.4)
        assert (layer.centroid_layer.output_stride, layer.centroid_layer.max_stride, layer.centroid_layer.max_instances) == (2, 8, 4)
        assert sorted(il.backend.model.param_shapes) == sorted(k[len("model.") :] for k in s.state_dict)
        assert [h.name for h in il.backend.model.heads] == ["SegmentationHead"]


def test_what_stays_refused(monkeypatch):
    from sleap_nn_amd.architectures.heads import SEGMENTATION_MODEL_TYPES, get_head
    from sleap_nn_amd.inference import predictor as P
    from sleap_nn_amd.inference.layers import CenteredInstanceMaskLayer, CentroidLayer, PostprocessConfig, TopDownSegmentationLayer
    from sleap_nn_amd.inference.loaders import load_model_assets

    c, s = load_model_assets(CENTROID_DIR), load_model_assets(SEG_DIR)
    monkeypatch.setattr(P, "HipBackend", lambda model, device: StubBackend(model))
    with pytest.raises(NotImplementedError, match="ground-truth-centroid"):  # the seg directory alone
        P._select_layer([s], "cuda:0", PostprocessConfig(), None)
    with pytest.raises(NotImplementedError, match="mask_output"):
        P._select_layer([c, s], "cuda:0", PostprocessConfig(), None, seg_kw={"mask_output": "polygon"})
    with pytest.raises(NotImplementedError, match="mask_output"):
        TopDownSegmentationLayer(CentroidLayer(StubBackend(), 2), CenteredInstanceMaskLayer(StubBackend(), 2), (32, 32), mask_output="both")
    s.preprocessing = dict(s.preprocessing, tiling={"enabled": True, "tile_size": 64, "overlap": 16})
    with pytest.raises(NotImplementedError, match="not centered_instance_segmentation"):
        P._select_layer([c, s], "cuda:0", PostprocessConfig(), None)
    with pytest.raises(Exception, match="bottomup_segmentation.*semantic_segmentation"):
        get_head("centered_instance_segmentation", {"segmentation": {"output_stride": 2}})
    assert SEGMENTATION_MODEL_TYPES == ("bottomup_segmentation", "semantic_segmentation")


def test_outputs_helpers_pass_the_stack_through():
    from sleap_nn_amd.inference.outputs import Outputs

    stack = torch.zeros((2, 3, 4, 5), dtype=torch.uint8)
    stack[1, 2, 3, 4] = 1
    out = Outputs(pred_masks=[[], []], pred_mask_stack=stack, pred_mask_counts=torch.tensor([0, 3], dtype=torch.int32))
    for o in (out.cpu(), out.slim(), out.detach()):
        assert torch.equal(o.pred_mask_stack, stack) and o.pred_mask_counts.tolist() == [0, 3] and o.pred_masks is out.pred_masks
    d = out.numpy()
    assert np.array_equal(d["pred_mask_stack"], stack.numpy()) and d["pred_mask_counts"].dtype == np.int32
    assert "pred_mask_stack=Tensor(2, 3, 4, 5)" in repr(out) and out.batch_size == 2
    assert Outputs().pred_mask_stack is None and Outputs().pred_mask_counts is None


@pytest.mark.parametrize("case", CASES)
def test_host_evaluator_takes_offset_entries(case):
    """Entries with an offset and a non-integer scale had no route into the evaluator: they are placed by the host ``place_crop_masks``."""
    from sleap_nn_amd.evaluation import MaskEvaluator, mask_pair_stats
    from sleap_nn_amd.inference.outputs import Outputs

    frames, decoded = recorded_entries(case)
    gt = np.zeros((3, 4) + FRAME_HW, dtype=np.uint8)
    k = 0
    for b, f in enumerate(frames):
        for j in range(len(f)):
            gt[b, j] = np.roll(clip_to_frame(decoded[k]), 3, axis=1)  # the prediction, shifted
            k += 1
    n_gt = np.array([len(f) for f in frames])
    stats = mask_pair_stats(Outputs(pred_masks=frames), gt, n_gt=n_gt)
    k = 0
    for b, f in enumerate(frames):
        iou, inter, pa, ga = stats[b]
        assert iou.shape == (len(f), len(f))
        for j in range(len(f)):
            p, g = clip_to_frame(decoded[k]), gt[b, j] != 0
            assert pa[j] == p.sum() and ga[j] == g.sum() and inter[j, j] == (p & g).sum()
            k += 1
    ev = MaskEvaluator()
    ev.add_batch(Outputs(pred_masks=frames), None, gt, n_gt=n_gt)
    assert len(ev) == 3 and [len(fr["pred_scores"]) for fr in ev._frames] == n_gt.tolist()
    assert np.array_equal(ev._frames[0]["pred_scores"], [d["score"] for d in frames[0]])
