"""Top-down instance segmentation on the GPU: ``ph_seg_place_crops`` (csrc/seg_kernels.hip) byte for byte against the host implementation of the same
contract, and the centroid + crop-mask pair on the two tiny run directories against the reference's recorded run (tests/golden/topdown_segmentation.npz,
tools/gen_topdown_seg_golden.py).

Score tolerance of the pair: 1e-4 absolute, the bound ``tests/test_gpu_segmentation.py`` applies to a run directory's scores -- the score is a mean of
probabilities, each within the project's standing 1e-4 of the reference's."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import _golden as G
from tests.test_topdown_seg_cpu import CASES, CENTROID_DIR, FRAME_HW, PARAMS, SEG_DIR, TDS, recorded_entries

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SCORE_ATOL = 1e-4


def _place_both(masks, pos, origins, extents, hw, P):
    """Device result (into a buffer pre-filled with 0xFF, through the C ABI) and the host result."""
    from sleap_nn_amd import _lib as L
    from sleap_nn_amd.inference.ops.segmentation import place_crop_masks

    want = place_crop_masks(masks, pos, origins, extents, hw, P)
    B = len(pos) // P
    m = torch.from_numpy(masks).to(DEV)
    p = torch.from_numpy(np.asarray(pos, dtype=np.int32)).to(DEV)
    g = torch.from_numpy(np.concatenate([origins, extents], axis=1).astype(np.int32)).to(DEV)
    out = torch.full((B, P, hw[0], hw[1]), 0xFF, dtype=torch.uint8, device=DEV)
    ptr = lambda t: C.c_void_p(t.data_ptr())
    L.check(L.lib().ph_seg_place_crops(ptr(m), masks.shape[0], masks.shape[1], masks.shape[2], ptr(p), ptr(g), B, P, hw[0], hw[1], ptr(out), L.current_stream_ptr()))
    again = place_crop_masks(m, p, torch.from_numpy(origins), torch.from_numpy(extents), hw, P)  # the op: device tensors in, a device tensor out
    assert again.is_cuda and torch.equal(again, out)
    return out.cpu().numpy(), want


def _random_masks(n, h, w, seed):
    return (np.random.default_rng(seed).random((n, h, w)) < 0.5).astype(np.uint8)


# frame 37 x 53 (no multiple of 16: most 16-byte chunks run over a row end, some over a slot end), B = 2, P = 3
ORIGINS = np.array([[-5, -3], [20, 9], [45, 30], [60, 40], [27, 14]])  # negative / inside / past the right and bottom edge / wholly outside / overlapping the second
POS = np.array([0, 1, 4, 2, -1, 3])  # frame 0: three crops, two of them overlapping; frame 1: one, an empty slot, one wholly outside


@pytest.mark.parametrize("mask_hw,extent", [((8, 8), (16, 16)), ((8, 8), (13, 11)), ((5, 7), (16, 16)), ((5, 7), (13, 11)), ((8, 8), (5, 3))])
def test_place_matches_host(mask_hw, extent):
    """Integer extents (16 x 16 from 8 x 8: factor 2), non-integer ones (13 x 11, and 16 x 16 from 5 x 7) and a down-sampling one (5 x 3: several source
    columns per step)."""
    masks = _random_masks(5, mask_hw[0], mask_hw[1], 3)
    got, want = _place_both(masks, POS, ORIGINS, np.tile(np.array([extent]), (5, 1)), (37, 53), 3)
    assert got.shape == (2, 3, 37, 53)
    assert np.array_equal(got, want)  # every byte written (none left 0xFF), zero for the empty slot and outside the crops
    assert not got[1, 1].any() and not got[1, 2].any() and got[0, 1].any() and got[0, 2].any()  # (the first crop is wholly outside at the smallest extent)


def test_place_per_crop_extents_aligned_width_and_values():
    """Every crop its own extent; a frame width that is a multiple of 16 (each chunk in one row); byte values are copied as they are."""
    masks = np.random.default_rng(4).integers(0, 256, (5, 8, 8)).astype(np.uint8)
    extents = np.array([[16, 16], [13, 11], [9, 20], [16, 16], [1, 1]])
    got, want = _place_both(masks, POS, ORIGINS, extents, (21, 64), 3)
    assert np.array_equal(got, want)
    got, want = _place_both(masks, np.full(6, -1), ORIGINS, extents, (5, 3), 3)  # nothing but empty slots, fewer than 16 bytes a plane
    assert np.array_equal(got, want) and not got.any()


def test_place_bad_records_are_empty():
    masks = _random_masks(3, 8, 8, 5)
    origins = np.array([[0, 0], [-(2**31), 0], [3, 2**31 - 1]])
    extents = np.array([[0, 16], [16, 16], [16, 70000]])  # an extent of 0, origins at the ends of int32, an extent beyond 65535
    got, want = _place_both(masks, np.array([0, 1, 2, 7]), origins, extents, (37, 53), 4)  # (and a list position beyond the crops)
    assert np.array_equal(got, want) and not got.any()


def test_place_slot_limits():
    from sleap_nn_amd import _lib as L

    masks = _random_masks(2, 8, 8, 6)
    pos = np.full(64, -1)
    pos[0], pos[63] = 0, 1
    got, want = _place_both(masks, pos, np.array([[1, 2], [30, 20]]), np.array([[16, 16], [13, 11]]), (37, 53), 64)
    assert np.array_equal(got, want) and got[0, 63].any()
    t = torch.zeros(1 << 16, dtype=torch.int32, device=DEV)
    p = C.c_void_p(t.data_ptr())
    for P in (65, 0):
        assert L.lib().ph_seg_place_crops(p, 1, 8, 8, p, p, 1, P, 8, 8, p, None) == L.PH_E_INVALID
        assert f"P={P}" in L.lib().ph_last_error().decode()
    assert L.lib().ph_seg_place_crops(p, 1, 8, 40000, p, p, 1, 1, 8, 8, p, None) == L.PH_E_INVALID  # crop side beyond 32767
    assert L.lib().ph_seg_place_crops(p, 1, 8, 8, p, p, 1, 64, 8192, 8192, p, None) == L.PH_E_INVALID  # 2^32 output bytes
    assert L.lib().ph_seg_place_crops(p, 1, 8, 8, p, p, 1, 1, 8, 8, C.c_void_p(t.data_ptr() + 4), None) == L.PH_E_INVALID  # output not 16-byte aligned


def test_place_past_2_31_bytes():
    """A 2.4-GB output: byte offsets beyond 2^31 (the kernel's indices are unsigned 32-bit).  Checked where the crops are and by the total."""
    from sleap_nn_amd.inference.ops.segmentation import place_crop_masks

    masks = _random_masks(2, 8, 8, 7) * 255
    H = W = 24500  # 4 x 24500^2 = 2.401e9
    origins, extents = np.array([[5, 7], [W - 10, H - 9]]), np.array([[16, 16], [13, 11]])
    pos = np.array([0, -1, -1, 1])
    out = place_crop_masks(torch.from_numpy(masks).to(DEV), torch.from_numpy(pos).to(DEV), origins, extents, (H, W), 4)
    small = place_crop_masks(masks, np.array([0, 1]), np.array([[5, 7], [40 - 10, 40 - 9]]), extents, (40, 40), 2)  # the same corners on a 40 x 40 frame
    assert np.array_equal(out[0, 0, :40, :40].cpu().numpy(), small[0, 0]) and np.array_equal(out[0, 3, H - 40 :, W - 40 :].cpu().numpy(), small[0, 1])
    assert small[0, 1].any()
    assert int(out.sum(dtype=torch.int64)) == int(small.sum(dtype=np.int64))  # nothing anywhere else
    del out
    torch.cuda.empty_cache()


# ---- the pair on the run directories ----------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def predictor():
    from sleap_nn_amd.inference.predictor import Predictor

    return Predictor.from_model_paths([CENTROID_DIR, SEG_DIR], device=DEV, batch_size=3, peak_threshold=PARAMS["peak_threshold"], max_instances=PARAMS["max_instances"],
                                      fg_threshold=PARAMS["fg_threshold"])


def _set_case(layer, case):
    from dataclasses import replace

    mh, mw = (None, None) if case == "plain" else PARAMS["sized_max_hw"]
    layer.centroid_layer.preprocess_config = replace(layer.centroid_layer.preprocess_config, max_height=mh, max_width=mw)


def _same_entries(a, b):
    assert [len(f) for f in a] == [len(f) for f in b]
    for fa, fb in zip(a, b):
        for da, db in zip(fa, fb):
            assert np.array_equal(da["mask"], db["mask"]) and da["score"] == db["score"] and da["scale"] == db["scale"] and da["offset"] == db["offset"]


@pytest.mark.parametrize("case", CASES)
def test_pair_matches_reference(predictor, case):
    from sleap_nn_amd.inference.layers import TopDownSegmentationLayer

    layer = predictor.layer
    assert isinstance(layer, TopDownSegmentationLayer) and predictor.replicas == []
    _set_case(layer, case)
    layer.place_masks = False
    out = layer.predict(torch.from_numpy(TDS["layer/frames"]))
    ref, _ = recorded_entries(case)
    unc = TDS[f"layer/{case}/uncertain"]
    assert out.pred_keypoints is None and out.pred_centroids is None and out.pred_mask_stack is None and out.preprocess_info is not None
    assert [len(f) for f in out.pred_masks] == [len(f) for f in ref] and out.pred_masks[2] == []  # the blob-free frame
    k = 0
    for b, (got, want) in enumerate(zip(out.pred_masks, ref)):
        for d, r in zip(got, want):  # same order
            assert d["scale"] == r["scale"] and d["offset"] == r["offset"], (case, b, d["scale"], r["scale"], d["offset"], r["offset"])
            assert d["mask"].dtype == bool and d["mask"].shape == r["mask"].shape
            diff = d["mask"] != r["mask"]
            print(case, "frame", b, "entry", k, "pixels that differ", int(diff.sum()), "outside the uncertain set", int((diff & ~unc[k]).sum()), "score", d["score"], "reference", r["score"])
            assert not (diff & ~unc[k]).any()
            assert abs(d["score"] - r["score"]) <= SCORE_ATOL
            k += 1


def test_host_nms_path_gives_the_same_entries(predictor):
    layer = predictor.layer
    _set_case(layer, "sized")
    layer.place_masks = True
    x = torch.from_numpy(TDS["layer/frames"])
    fast = layer.predict(x)
    layer.centroid_nms, layer.centroid_nms_threshold = True, 0.99  # (no two recorded crops overlap that much: NMS drops nothing)
    try:
        slow = layer.predict(x)
    finally:
        layer.centroid_nms = False
    _same_entries(fast.pred_masks, slow.pred_masks)
    assert torch.equal(fast.pred_mask_stack, slow.pred_mask_stack) and torch.equal(fast.pred_mask_counts, slow.pred_mask_counts)


@pytest.mark.parametrize("case", CASES)
def test_stack_equals_host_placement_and_feeds_the_evaluator(predictor, case):
    from sleap_nn_amd.evaluation import mask_pair_stats
    from sleap_nn_amd.inference.ops.segmentation import stack_pred_masks
    from sleap_nn_amd.inference.outputs import Outputs

    layer = predictor.layer
    _set_case(layer, case)
    layer.place_masks = True
    out = layer.predict(torch.from_numpy(TDS["layer/frames"]))
    P = PARAMS["max_instances"]
    assert out.pred_mask_stack.is_cuda and out.pred_mask_stack.dtype == torch.uint8 and tuple(out.pred_mask_stack.shape) == (3, P) + FRAME_HW
    assert out.pred_mask_counts.dtype == torch.int32 and out.pred_mask_counts.tolist() == [len(f) for f in out.pred_masks]
    want, counts = stack_pred_masks(out.pred_masks, FRAME_HW, P)
    assert np.array_equal(out.pred_mask_stack.cpu().numpy(), want) and want[:2].any() and not want[2].any()
    # ground truth: the recorded decode of each entry, shifted; integers, so device and host evaluator agree exactly
    gt = np.roll(want, 4, axis=-1)
    dev_stats = mask_pair_stats(out, torch.from_numpy(gt).to(DEV), n_gt=counts)
    host_stats = mask_pair_stats(Outputs(pred_masks=out.pred_masks), gt, n_gt=counts)
    for (i0, n0, p0, g0), (i1, n1, p1, g1) in zip(dev_stats, host_stats):
        assert np.array_equal(n0, n1) and np.array_equal(p0, p1) and np.array_equal(g0, g1) and np.array_equal(i0, i1)
    assert dev_stats[0][1].shape == (counts[0], counts[0]) and dev_stats[0][1].diagonal().min() > 0
    empty = layer.predict(torch.from_numpy(TDS["layer/frames"][2:]))  # a batch without a centroid
    assert empty.pred_masks == [[]] and tuple(empty.pred_mask_stack.shape) == (1, P) + FRAME_HW and not empty.pred_mask_stack.any() and empty.pred_mask_counts.tolist() == [0]


def test_predictor_runs_two_batches(predictor):
    layer = predictor.layer
    _set_case(layer, "plain")
    layer.place_masks = False
    frames = TDS["layer/frames"]
    predictor.batch_size = 2
    try:
        outs = predictor.predict(frames)
    finally:
        predictor.batch_size = 3
    assert len(outs) == 2 and outs[0].frame_indices.tolist() == [0, 1] and outs[1].frame_indices.tolist() == [2]
    direct = layer.predict(torch.from_numpy(frames))
    _same_entries(outs[0].pred_masks + outs[1].pred_masks, direct.pred_masks)
