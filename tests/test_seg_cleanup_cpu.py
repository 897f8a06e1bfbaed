"""Mask cleanup (largest component + hole fill) without a GPU: the host path against the reference's recorded results
(tests/golden/seg_cleanup.npz, tools/gen_seg_cleanup_golden.py) -- every mask, centre and score equal --, ``clean_label_map`` against SciPy on
seeded random label maps, the new layer and its routing, and ``mask_cleanup=False`` against the uncleaned goldens."""
import json
import os

import numpy as np
import pytest
import torch

from tests import _golden as G
from tests.test_segmentation_cpu import GROUP_NAMES as PLAIN_NAMES
from tests.test_segmentation_cpu import StubBackend, _case as plain_case, check_grouping, group_kwargs

CL = G.load("seg_cleanup.npz")
NAMES = json.loads(str(CL["group/names"]))
LAYER_NAMES = json.loads(str(CL["layer/names"]))


def case(name):
    p = json.loads(str(CL[f"group/{name}/params"]))
    return tuple(torch.from_numpy(CL[f"group/{name}/{k}"]) for k in ("fg", "hm", "off")), p


def check_cleaned(name, g, p):
    """``g`` (a ``Grouping`` with holes) against the reference's record: centres, then per instance the mask bit for bit, the area, the centre and the score."""
    assert g.holes is not None and len(g.holes) == g.labels.shape[0]
    for b in range(g.labels.shape[0]):
        assert np.array_equal(g.centers[b], CL[f"group/{name}/{b}/peaks"]), (name, b)
        assert np.abs(g.scores[b].astype(np.float64) - CL[f"group/{name}/{b}/peak_vals"]).max(initial=0) <= 1e-6
        ref = CL[f"group/{name}/{b}/masks"]
        inst = g.instances(b, p["output_stride"])
        assert len(inst) == len(ref), (name, b, len(inst), len(ref))
        kept = np.nonzero(g.counts[b] > 0)[0]
        for i, d in enumerate(inst):
            assert d["mask"].dtype == bool and np.array_equal(d["mask"], ref[i]), (name, b, i, int((d["mask"] != ref[i]).sum()))
            assert int(g.counts[b][kept[i]]) == int(ref[i].sum()), (name, b, i)
            assert d["center"] == tuple(CL[f"group/{name}/{b}/inst_centers"][i])
            assert abs(d["score"] - CL[f"group/{name}/{b}/inst_scores"][i]) <= 1e-6
        hol = g.holes[b]
        assert hol.dtype == np.int32 and hol.ndim == 2 and hol.shape[1] == 2
        if len(hol):  # instance-major, raster order inside an instance; a hole is never a pixel of its own component
            key = hol[:, 1].astype(np.int64) * g.labels[b].size + hol[:, 0]
            assert np.all(np.diff(key) > 0)
            assert np.all(g.labels[b].reshape(-1)[hol[:, 0]] != hol[:, 1])


def random_label_maps():
    """Seeded label maps for ``clean_label_map``: (name, labels (h, w) int32, n).  Speckle at several densities (many fragments, ties, holes that nest), sizes
    that are no multiple of the 16 x 64 tile or the 64-column word, a label nobody carries, one row and one column."""
    out = []
    for seed, (h, w, n, density) in enumerate([(33, 70, 3, 0.75), (48, 130, 5, 0.6), (17, 64, 1, 0.8), (64, 65, 2, 0.9), (1, 90, 2, 0.7), (75, 1, 2, 0.7), (40, 40, 200, 0.5)]):
        g = np.random.default_rng(1000 + seed)
        lab = g.integers(0, max(1, n - 1) if n > 2 else n, size=(h, w)).astype(np.int32)  # (n > 2: the last label stays unused)
        coarse = g.integers(0, max(1, n - 1) if n > 2 else n, size=((h + 7) // 8, (w + 7) // 8))
        big = np.kron(coarse, np.ones((8, 8), dtype=np.int64))[:h, :w]
        lab = np.where(g.random((h, w)) < 0.7, big, lab).astype(np.int32)  # blocks of one label with speckle of the others
        lab[g.random((h, w)) > density] = -1
        out.append((f"rand{seed}_{h}x{w}_n{n}", lab, n))
    return out


RANDOM_MAPS = random_label_maps()


def masks_of(cleaned, holes, n):
    out = []
    for k in range(n):
        m = cleaned == k
        m.reshape(-1)[holes[holes[:, 1] == k, 0]] = True
        out.append(m)
    return out


@pytest.mark.parametrize("name", NAMES)
def test_host_cleanup_reproduces_reference(name):
    from sleap_nn_amd.inference.ops.segmentation import group_instances_from_offsets

    (fg, hm, off), p = case(name)
    check_cleaned(name, group_instances_from_offsets(fg, hm, off, mask_cleanup=True, **group_kwargs(p)), p)


def test_golden_covers_the_required_cases():
    assert {"ring_around", "nested_rings", "equal_fragments", "diagonal", "cavities", "serpentine", "odd_13x67", "one_row", "one_column", "batch3", "gate_topk",
            "many_centres", "big_ring"} <= set(NAMES)
    m = CL["group/ring_around/0/masks"]
    assert (m[0] & m[1]).sum() == 30  # the ring fills over the inner instance, which keeps its own mask
    assert CL["group/serpentine/fg"].shape[-2:] == (40, 72) and CL["group/big_ring/0/masks"].shape[-2:] == (640, 640)
    assert len(CL["group/many_centres/0/peaks"]) > 127
    assert len(CL["group/batch3/1/masks"]) == 0 and len(CL["group/batch3/2/masks"]) == 0 and len(CL["group/batch3/0/masks"]) == 2
    p = json.loads(str(CL["group/gate_topk/params"]))
    assert p["distance_gate_alpha"] is not None and p["max_instances"] == 2


@pytest.mark.parametrize("name,lab,n", RANDOM_MAPS, ids=[m[0] for m in RANDOM_MAPS])
def test_clean_label_map_matches_scipy(name, lab, n):
    ndi = pytest.importorskip("scipy.ndimage")
    from sleap_nn_amd.inference.ops.segmentation import clean_label_map

    cleaned, holes, areas = clean_label_map(lab, n)
    got = masks_of(cleaned, holes, n)
    assert areas.shape == (n,) and cleaned.shape == lab.shape
    for k in range(n):
        mask = lab == k
        if not mask.any():
            assert areas[k] == 0 and not got[k].any()
            continue
        cc, m = ndi.label(mask)
        if m > 1:
            counts = np.bincount(cc.ravel())
            counts[0] = 0
            mask = cc == int(counts.argmax())
        ref = ndi.binary_fill_holes(mask)
        assert np.array_equal(cleaned == k, mask), (name, k)
        assert np.array_equal(got[k], ref), (name, k)
        assert areas[k] == ref.sum()


def _raw(prefix):
    return {"SegmentationHead": torch.from_numpy(CL[f"{prefix}/fg"])[None, None], "InstanceCenterHead": torch.from_numpy(CL[f"{prefix}/hm"])[None, None],
            "CenterOffsetHead": torch.from_numpy(CL[f"{prefix}/off"])[None]}


@pytest.mark.parametrize("name", LAYER_NAMES)
def test_layer_applies_the_area_floor_to_the_cleaned_mask(name):
    from sleap_nn_amd.inference.layers import CleanupSegmentationLayer
    from sleap_nn_amd.inference.preprocess_info import PreprocInfo

    orig, proc, eff, iscale, stride = json.loads(str(CL["layer/info"]))
    area, res = name.split("/")
    layer = CleanupSegmentationLayer(StubBackend(), stride, min_mask_area=int(area[1:]), full_res_masks=res == "full")
    assert layer.mask_cleanup is True
    info = PreprocInfo(original_size=tuple(orig), processed_size=tuple(proc), eff_scale=torch.tensor([eff], dtype=torch.float32), input_scale=iscale, output_stride=stride)
    got = layer.postprocess(_raw("layer"), info).pred_masks[0]
    assert len(got) == int(CL[f"layer/{name}/n"])
    for i, d in enumerate(got):
        ref_mask, meta = CL[f"layer/{name}/{i}/mask"], CL[f"layer/{name}/{i}/meta"]
        assert d["mask"].dtype == bool and d["mask"].shape == ref_mask.shape and np.array_equal(d["mask"], ref_mask), (name, i)
        assert abs(d["score"] - meta[0]) <= 1e-6
        assert tuple(d["scale"]) == (meta[1], meta[2]) and tuple(d["offset"]) == (meta[3], meta[4])


@pytest.mark.parametrize("knob,value", [("mask_cleanup_radius", 2), ("merge_fragments", True), ("mask_output", "polygon"), ("mask_output", "both")])
def test_new_layer_still_refuses_the_other_knobs(knob, value):
    from sleap_nn_amd.inference.layers import CleanupSegmentationLayer, SegmentationLayer

    with pytest.raises(NotImplementedError, match=knob):
        CleanupSegmentationLayer(StubBackend(), 2, **{knob: value})
    with pytest.raises(NotImplementedError, match="mask_cleanup"):
        SegmentationLayer(StubBackend(), 2, mask_cleanup=True)
    assert issubclass(CleanupSegmentationLayer, SegmentationLayer)


@pytest.mark.parametrize("cleanup,cls_name", [(True, "CleanupSegmentationLayer"), (False, "SegmentationLayer")])
def test_select_layer_routes_on_the_knob(cleanup, cls_name, monkeypatch):
    from sleap_nn_amd.inference import predictor as P
    from sleap_nn_amd.inference.layers import PostprocessConfig
    from sleap_nn_amd.inference.loaders import load_model_assets

    a = load_model_assets(os.path.join(G.GOLDEN_DIR, "ckpt_dirs", "tiny_bottomup_segmentation"))
    monkeypatch.setattr(P, "HipBackend", lambda model, device: StubBackend(model))
    layer = P._select_layer([a], "cuda:0", PostprocessConfig(peak_threshold=0.2), 5, seg_kw={"mask_cleanup": cleanup, "min_mask_area": 7, "distance_gate_alpha": 1.5})
    assert type(layer).__name__ == cls_name and layer.mask_cleanup is cleanup
    assert layer.min_mask_area == 7 and layer.max_instances == 5 and layer.distance_gate_alpha == 1.5 and layer.output_stride == 2
    with pytest.raises(NotImplementedError, match="mask_cleanup_radius"):
        P._select_layer([a], "cuda:0", PostprocessConfig(), None, seg_kw={"mask_cleanup": True, "mask_cleanup_radius": 1})


@pytest.mark.parametrize("name", PLAIN_NAMES)
def test_cleanup_off_is_the_recorded_uncleaned_result(name):
    from sleap_nn_amd.inference.ops.segmentation import group_instances_from_offsets

    (fg, hm, off), p = plain_case(name)
    g = group_instances_from_offsets(fg, hm, off, mask_cleanup=False, **group_kwargs(p))
    assert g.holes is None
    check_grouping(name, g, p)


def test_abi_declares_the_cleanup_entry_points():
    import re

    from sleap_nn_amd import _lib as L

    header = open(os.path.join(os.path.dirname(G.GOLDEN_DIR), "..", "include", "posehip.h")).read()
    assert int(re.search(r"^#define\s+PH_VERSION\s+(\d+)", header, re.M).group(1)) >= 115
    assert {"ph_seg_cleanup", "ph_seg_cleanup_scratch_bytes"} <= set(L.SIGNATURES)
    lib = L.lib()
    assert lib.ph_seg_cleanup_scratch_bytes(0, 4, 4, 8, 0) == 0 and lib.ph_seg_cleanup_scratch_bytes(1, 4, 4, 8, 0) > 5 * 16 * 4
