"""Mask cleanup on the GPU: ``ph_seg_cleanup`` (csrc/seg_cleanup_kernels.hip) behind ``group_instances_from_offsets(mask_cleanup=True)`` against the
reference's recorded results -- every mask, area, centre and score equal --, run-to-run identity, the host implementation on seeded random label maps
through the C ABI, the capacity retries, and a run directory through ``Predictor``.  Goldens: tools/gen_seg_cleanup_golden.py."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests import _golden as G
from tests.test_segmentation_cpu import group_kwargs
from tests.test_seg_cleanup_cpu import CL, NAMES, RANDOM_MAPS, case, check_cleaned

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _group(name, **kw):
    from sleap_nn_amd.inference.ops.segmentation import group_instances_from_offsets

    (fg, hm, off), p = case(name)
    return group_instances_from_offsets(fg.to(DEV), hm.to(DEV), off.to(DEV), mask_cleanup=True, **group_kwargs(p), **kw), p


@pytest.mark.parametrize("name", NAMES)
def test_device_cleanup_reproduces_reference(name):
    """Default capacities: 'many_centres' comes back once for two-byte labels; 'big_ring' floods its box in the scratch pool."""
    g, p = _group(name)
    check_cleaned(name, g, p)
    n = max(len(c) for c in g.centers)
    assert g.labels.dtype == (np.int8 if n <= 127 else np.int16)


@pytest.mark.parametrize("name", ["nested_rings", "serpentine", "many_centres", "batch3"])
def test_repeatable_and_on_another_stream(name):
    g0, p = _group(name)
    s = torch.cuda.Stream(DEV)
    with torch.cuda.stream(s):
        g1, _ = _group(name)
    check_cleaned(name, g1, p)
    assert np.array_equal(g0.labels, g1.labels)
    for b in range(len(g0.centers)):
        assert np.array_equal(g0.holes[b], g1.holes[b]) and np.array_equal(g0.counts[b], g1.counts[b])


def test_retry_on_small_capacities():
    """One hole pair per frame, no pool at all, a candidate list and a label width that are too small: each comes back with room."""
    g, p = _group("nested_rings", hole_cap=1)
    check_cleaned("nested_rings", g, p)
    g, p = _group("many_centres", hole_cap=7, cap=16, max_centers=8)
    check_cleaned("many_centres", g, p)
    g, p = _group("big_ring", hole_cap=16, pool_words=0)
    check_cleaned("big_ring", g, p)


def _cleanup_abi(lab, n, label_dtype):
    """``ph_seg_cleanup`` on one label map through the C ABI (outputs pre-filled with a pattern): (cleaned, holes, areas)."""
    from sleap_nn_amd import _lib as L

    h, w = lab.shape
    lt = torch.from_numpy(lab.astype(label_dtype))[None].to(DEV)
    out = torch.full_like(lt, 77)
    cap = max(1, h * w)
    counts = torch.tensor([n, 0], dtype=torch.int32, device=DEV)
    rec = torch.full((2 * n + 2,), -5, dtype=torch.int32, device=DEV)
    holes = torch.full((1, cap, 2), -7, dtype=torch.int32, device=DEV)
    pool = 2 * (h + 2) * ((w + 2 + 63) // 64)
    need = int(L.lib().ph_seg_cleanup_scratch_bytes(1, h, w, n, pool))
    scratch = torch.empty((need + 7) // 8, dtype=torch.int64, device=DEV)
    p = lambda t: C.c_void_p(t.data_ptr())
    L.check(L.lib().ph_seg_cleanup(p(lt), 1, h, w, p(counts), n, lt.element_size(), p(out), p(rec), p(holes), cap, pool, p(scratch), need, L.current_stream_ptr()))
    torch.cuda.synchronize()
    rec = rec.cpu().numpy()
    total = int(rec[2 * n])
    assert int(rec[n : 2 * n].sum()) == total and rec[2 * n + 1] <= pool
    hol = holes[0].cpu().numpy()
    assert np.all(hol[total:] == -7)
    return out[0].cpu().numpy(), hol[:total], rec[:n]


@pytest.mark.parametrize("name,lab,n", RANDOM_MAPS, ids=[m[0] for m in RANDOM_MAPS])
def test_device_equals_host_on_random_label_maps(name, lab, n):
    from sleap_nn_amd.inference.ops.segmentation import clean_label_map

    ref_clean, ref_holes, ref_areas = clean_label_map(lab, n)
    for dt in ([np.int8] if n <= 127 else []) + [np.int16, np.int32]:
        cleaned, holes, areas = _cleanup_abi(lab, n, dt)
        assert cleaned.dtype == dt and np.array_equal(cleaned, ref_clean), (name, dt)
        assert np.array_equal(holes, ref_holes), (name, dt)
        assert np.array_equal(areas, ref_areas), (name, dt)


def test_c_abi_rejects_bad_arguments():
    from sleap_nn_amd import _lib as L

    t = torch.zeros(1 << 16, dtype=torch.int32, device=DEV)
    u = torch.zeros(64, dtype=torch.int32, device=DEV)
    p, q = C.c_void_p(t.data_ptr()), C.c_void_p(u.data_ptr())
    lib = L.lib()
    assert lib.ph_seg_cleanup(p, 1, 4, 4, q, 8, 1, p, q, q, 4, 0, p, 1 << 18, None) == L.PH_E_INVALID  # in place
    assert lib.ph_seg_cleanup(q, 1, 4, 4, q, 200, 1, p, q, q, 4, 0, p, 1 << 18, None) == L.PH_E_INVALID  # 200 centres in one-byte labels
    assert lib.ph_seg_cleanup(q, 1, 4, 40000, q, 8, 1, p, q, q, 4, 0, p, 1 << 18, None) == L.PH_E_INVALID  # a side beyond 32767
    assert lib.ph_seg_cleanup(q, 1, 4, 4, q, 8, 1, p, q, q, 4, 0, p, 8, None) == L.PH_E_WORKSPACE


def test_run_directory_through_predictor():
    from sleap_nn_amd.inference.layers import CleanupSegmentationLayer
    from sleap_nn_amd.inference.predictor import Predictor

    pred = Predictor.from_model_paths([os.path.join(G.GOLDEN_DIR, "ckpt_dirs", "tiny_bottomup_segmentation")], device=DEV, batch_size=2, mask_cleanup=True)
    assert isinstance(pred.layer, CleanupSegmentationLayer)
    outs = pred.predict(CL["rundir/frames"])
    assert len(outs) == 1 and len(outs[0].pred_masks) == 2
    for b in range(2):  # (the generator asserted an empty uncertain set: no pixel is excused)
        got = outs[0].pred_masks[b]
        ref_masks, ref_scores, ref_scales = CL[f"rundir/{b}/masks"], CL[f"rundir/{b}/scores"], CL[f"rundir/{b}/scales"]
        assert len(got) == int(CL[f"rundir/{b}/n"]) >= 2
        for i, d in enumerate(got):
            assert abs(d["score"] - ref_scores[i]) <= 1e-4, (b, i, d["score"], ref_scores[i])
            assert tuple(d["scale"]) == tuple(ref_scales[i]) and d["mask"].shape == ref_masks[i].shape
            print("frame", b, "instance", i, "pixels that differ", int((d["mask"] != ref_masks[i]).sum()))
            assert np.array_equal(d["mask"], ref_masks[i]), (b, i)
