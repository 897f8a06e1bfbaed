"""Mask evaluation on the GPU: ``ph_mask_pair_stats`` and ``ph_mask_boundary`` (csrc/eval_kernels.hip) through ``sleap_nn_amd.evaluation`` against the
reference's recorded results (tests/golden/seg_evaluation.npz), to the bars of tests/test_seg_evaluation_cpu.py: integer tables and boundary masks equal,
two runs bit-identical, padding slots zero, the evaluators' dictionaries as on the host."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests.test_seg_evaluation_cpu import (PAIR_CASES, RTOL, boundary_case, check_dict, check_frames, check_tables, feed_mask_evaluator, feed_semantic_evaluator,
                                           matched_pairs, pair_case)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LABEL_DTYPES = {1: torch.int8, 2: torch.int16, 4: torch.int32}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _tables(name, form, width=1):
    from sleap_nn_amd.evaluation import mask_pair_tables

    c = pair_case(name)
    pred = dev(c["pred"]) if form == "stack" else dev(c["labels"]).to(LABEL_DTYPES[width])
    out = mask_pair_tables(pred, dev(c["gt"]), c["n_pred"], c["n_gt"], c["s"])
    assert all(t.is_cuda and t.dtype == torch.int32 for t in out)
    return [t.cpu().numpy() for t in out]


@pytest.mark.parametrize("form,width", [("stack", 0), ("label", 1), ("label", 2), ("label", 4)])
@pytest.mark.parametrize("name", PAIR_CASES)
def test_pair_stats_kernel(name, form, width):
    first = _tables(name, form, width)
    check_tables(name, form, *first)  # the recorded tables are 0 in the padding slots
    c = pair_case(name)
    for b in range(len(c["n_pred"])):
        assert not first[0][b, c["n_pred"][b] :].any() and not first[0][b, :, c["n_gt"][b] :].any() and not first[1][b, c["n_pred"][b] :].any() and not first[2][b, c["n_gt"][b] :].any()
    for a, b in zip(first, _tables(name, form, width)):
        assert a.tobytes() == b.tobytes()


def test_padding_slots_are_never_read():
    """Masks and labels at or beyond a frame's counts hold foreground here: they must not count."""
    from sleap_nn_amd.evaluation import mask_pair_tables

    c = pair_case("a")
    pred, gt, labels = c["pred"].copy(), c["gt"].copy(), c["labels"].copy()
    for b in range(4):
        pred[b, c["n_pred"][b] :] = True
        gt[b, c["n_gt"][b] :] = True
        labels[b][labels[b] < 0] = c["n_pred"][b]  # the first label that is out of range
    check_tables("a", "stack", *(t.cpu().numpy() for t in mask_pair_tables(dev(pred), dev(gt), c["n_pred"], c["n_gt"], 1)))
    check_tables("a", "label", *(t.cpu().numpy() for t in mask_pair_tables(dev(labels), dev(gt), c["n_pred"], c["n_gt"], 1)))


@pytest.mark.parametrize("name", ["a", "b1", "b2"])
def test_pair_stats_frames_and_matching(name):
    from sleap_nn_amd.evaluation import mask_pair_stats

    c = pair_case(name)
    check_frames(name, "stack", mask_pair_stats(dev(c["pred"]), dev(c["gt"]), c["n_pred"], c["n_gt"], c["s"]))
    s = torch.cuda.Stream(DEV)
    with torch.cuda.stream(s):
        stats = mask_pair_stats(dev(c["labels"]), dev(c["gt"]), c["n_pred"], c["n_gt"], c["s"])
    check_frames(name, "label", stats)


@pytest.mark.parametrize("name", ["a", "d", "d_wide"])
def test_boundary_kernel(name):
    from sleap_nn_amd.evaluation import mask_boundary

    masks, d, want = boundary_case(name)  # a: d = 1; d: d = 7; d_wide: d = 18, wider than most blobs, whose boundary is the whole mask
    got = mask_boundary(dev(masks), d)
    assert got.is_cuda and got.dtype == torch.uint8
    assert np.array_equal(got.cpu().numpy(), want.astype(np.uint8))
    assert np.array_equal(mask_boundary(dev(masks.astype(np.uint8) * 255), d).cpu().numpy(), want.astype(np.uint8))  # any nonzero byte is foreground


def test_boundary_kernel_unaligned_rows():
    """Odd widths and an odd base address: the byte paths of the loads and stores, against the host implementation of the same contract."""
    from sleap_nn_amd.evaluation import mask_boundary

    g = np.random.default_rng(5)
    for (n, h, w), d in (((3, 33, 47), 2), ((2, 21, 16), 1), ((1, 40, 131), 3)):
        m = g.random((n, h, w)) > 0.08
        want = mask_boundary(m, d).astype(np.uint8)
        assert np.array_equal(mask_boundary(dev(m), d).cpu().numpy(), want)
        flat = torch.zeros(n * h * w + 1, dtype=torch.uint8, device=DEV)
        flat[1:] = dev(m.astype(np.uint8)).reshape(-1)
        assert np.array_equal(mask_boundary(flat[1:].view(n, h, w), d).cpu().numpy(), want)


@pytest.mark.parametrize("name", ["a", "b1", "b2", "d"])
def test_boundary_iou_of_matched_pairs(name):
    from sleap_nn_amd.evaluation import boundary_iou

    pm, gm, want = matched_pairs(name, "stack")
    np.testing.assert_allclose(boundary_iou(dev(pm), dev(gm)), want, rtol=RTOL, atol=0)


@pytest.mark.parametrize("form", ["label", "stack"])
def test_mask_evaluator_on_device(form):
    from sleap_nn_amd.evaluation import MaskEvaluator

    ev = feed_mask_evaluator(MaskEvaluator(0.5), to=dev, form=form)
    check_dict(ev.mask_metrics(), "ev/mask_metrics/", exact=("per_size/",))
    check_dict(ev.mask_voc_metrics(), "ev/mask_voc_metrics/", exact=("mask_voc.",))


def test_semantic_evaluator_on_device():
    from sleap_nn_amd.evaluation import SemanticEvaluator

    check_dict(feed_semantic_evaluator(SemanticEvaluator(), to=dev).semantic_metrics(), "ev/semantic_metrics/")


def test_c_abi_rejects_bad_arguments():
    from sleap_nn_amd import _lib as L

    lib = L.lib()
    t = torch.zeros(65 * 64 + 4096, dtype=torch.int32, device=DEV)
    p = C.c_void_p(t.data_ptr())
    for P, G, form, stride in ((65, 1, 0, 1), (1, 65, 0, 1), (0, 1, 0, 1), (1, 1, 3, 1), (1, 1, 0, 0)):
        assert lib.ph_mask_pair_stats(p, form, P, 4, 4, stride, p, G, 4, 4, 1, p, p, p, p, p, None) == L.PH_E_INVALID
    assert lib.ph_mask_boundary(p, 1, 4, 4, 0, C.c_void_p(t.data_ptr() + 64), p, 1024, None) == L.PH_E_INVALID
    assert lib.ph_mask_boundary(p, 1, 4, 4, 1, C.c_void_p(t.data_ptr() + 64), C.c_void_p(t.data_ptr() + 128), 2, None) == L.PH_E_WORKSPACE
