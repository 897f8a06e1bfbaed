"""Fragment merge (the RAG of ``merge_instances``) without a GPU: the host path against the reference's recorded results (tests/golden/seg_merge.npz,
tools/gen_seg_merge_golden.py) -- edges with their integer overlaps, affinities within 1e-7, every merged mask, centre and score equal for both methods --,
``merge_tables_host`` against a brute-force dilation on seeded random label maps, the agglomerations on hand-made edge sets, the new layer and its routing,
the refusals, and ``merge_fragments=False`` against the unmerged goldens.

The bound on an affinity is 1e-7 absolute: a tenth of the 1e-6 margin the generator asserts for every recorded decision, so any result inside it makes
the reference's decisions."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from tests import _golden as G
from tests.test_segmentation_cpu import GROUP_NAMES as PLAIN_NAMES
from tests.test_segmentation_cpu import StubBackend, _case as plain_case, check_grouping, group_kwargs

MG = G.load("seg_merge.npz")
NAMES = json.loads(str(MG["group/names"]))
LAYER_NAMES = json.loads(str(MG["layer/names"]))
AFF_TOL = 1e-7
METHODS = ("greedy", "multicut")


def case(name):
    p = json.loads(str(MG[f"group/{name}/params"]))
    return tuple(torch.from_numpy(MG[f"group/{name}/{k}"]) for k in ("fg", "hm", "off")), p


def merge_kwargs(p, method=None):
    return dict(merge_fragments=True, merge_method=method or p["merge_method"], merge_thresholds=tuple(p["merge_thresholds"]), merge_w_valley=p["merge_w_valley"],
                merge_w_offset=p["merge_w_offset"], merge_dilate=p["merge_dilate"])


def check_merged(name, g, p, method, trace, worst=None):
    """``g`` (a merged ``Grouping``) and its trace against the reference's record of ``method``: the graph's edges (instance numbering of the reference: centres
    with pixels), then per merged instance the mask bit for bit, the count, the centre and the score.  ``worst`` (a list) collects the affinity differences."""
    assert g.members is not None and len(g.members) == g.labels.shape[0] == len(trace)
    for b in range(g.labels.shape[0]):
        pre = f"group/{name}/{b}"
        ref_masks = MG[f"{pre}/{method}/masks"]
        inst = g.instances(b, p["output_stride"])
        assert len(inst) == len(ref_masks), (name, b, method, len(inst), len(ref_masks))
        kept = np.nonzero(g.counts[b] > 0)[0]
        for i, d in enumerate(inst):
            assert d["mask"].dtype == bool and np.array_equal(d["mask"], ref_masks[i]), (name, b, method, i)
            assert int(g.counts[b][kept[i]]) == int(ref_masks[i].sum())
            assert d["center"] == tuple(MG[f"{pre}/{method}/centers"][i])
            assert d["score"] == MG[f"{pre}/{method}/scores"][i]  # (a float32 peak value, copied)
        members = [m for m in g.members[b]]
        assert sorted(k for m in members for k in m) == list(range(len(MG[f"{pre}/peaks"]))) and all(m == sorted(m) for m in members)
        assert [m[0] for m in members] == sorted(m[0] for m in members)  # ordered by smallest member
        ref_edges, ref_aff = MG[f"{pre}/edges"], MG[f"{pre}/aff"]
        if method == "none" or int(MG[f"{pre}/n_inst"]) < 2:
            assert not trace[b]
            continue
        # centre index -> the reference's instance index (centres with pixels before the merge)
        with_pixels = sorted(k for m, c in zip(members, g.counts[b]) if c > 0 for k in m)
        inst_of = {k: i for i, k in enumerate(with_pixels)}
        got = [(inst_of[i], inst_of[j], ov, a) for (i, j, a), (_i, _j, ov, *_r) in zip(trace[b]["edges"], trace[b]["detail"])]
        assert [e[:3] for e in got] == [tuple(r) for r in ref_edges.tolist()], (name, b, "edges or overlaps differ")
        diff = np.abs(np.array([e[3] for e in got]) - ref_aff)
        if worst is not None:
            worst.extend(diff.tolist())
        assert diff.max(initial=0) <= AFF_TOL, (name, b, diff.max())


@pytest.mark.parametrize("name", NAMES)
def test_host_merge_reproduces_reference(name):
    from sleap_nn_amd.inference.ops.segmentation import group_instances_from_offsets

    (fg, hm, off), p = case(name)
    for method in sorted(set(METHODS) | {p["merge_method"]}):
        trace = []
        g = group_instances_from_offsets(fg, hm, off, **group_kwargs(p), **merge_kwargs(p, method), merge_trace=trace)
        check_merged(name, g, p, method, trace)


def test_golden_covers_the_required_cases():
    assert {"ridge_vs_valley", "chain", "dilate_1", "dilate_2", "dilate_3", "once_per_instance", "odd_13x67", "one_row", "one_column", "tiles_40x72", "image_edges",
            "noisy_offsets", "noisy_gated", "contact_only", "thresholds_05", "method_none", "many_centres", "batch4"} <= set(NAMES)
    assert MG["group/ridge_vs_valley/fg"].shape[-2:] == (24, 40) and len(MG["group/ridge_vs_valley/0/peaks"]) == 5
    assert sorted(MG["group/ridge_vs_valley/0/greedy/masks"].sum((1, 2)).tolist()) == [16, 56, 56, 112]
    assert len(MG["group/chain/0/greedy/masks"]) != len(MG["group/chain/0/multicut/masks"])  # the two methods disagree on the chain
    assert [len(MG[f"group/dilate_{d}/0/edges"]) for d in (1, 2, 3)] == [1, 3, 4]  # one and two cells apart, and a diagonal touch at d = 2
    assert MG["group/tiles_40x72/fg"].shape[-2:] == (40, 72)
    assert len(MG["group/many_centres/0/peaks"]) > 127 and len(MG["group/many_centres/0/edges"]) > 256
    assert [int(MG[f"group/batch4/{b}/n_inst"]) for b in range(4)] == [5, 0, 0, 1]
    p = json.loads(str(MG["group/noisy_gated/params"]))
    assert p["distance_gate_alpha"] is not None
    assert MG["group/noisy_gated/0/greedy/masks"].sum() < MG["group/noisy_offsets/0/greedy/masks"].sum()  # gated pixels are no members
    rp = json.loads(str(MG["rundir/params"]))
    assert rp["merged"] is True and min(rp["edges"]) > 0


def random_label_maps():
    """Seeded label maps for the pair tables: (name, labels (h, w) int32, n, dilate).  Blocks of one label with speckle of the others (a pixel then sees many
    labels: the de-duplication), pure speckle at d = 4 (up to 40 distinct neighbours), sizes that are no multiple of the 16 x 64 tile, a label nobody carries,
    one row, one column, more centres than the device accumulates in LDS (64) and than one-byte labels hold (127)."""
    out = []
    spec = [(33, 70, 3, 0.75, 1), (48, 130, 5, 0.6, 2), (17, 64, 64, 0.8, 3), (40, 72, 65, 0.9, 4), (1, 41, 3, 0.8, 2), (37, 1, 3, 0.8, 1), (13, 67, 200, 0.7, 4),
            (20, 20, 30, 1.0, 4)]
    for seed, (h, w, n, density, d) in enumerate(spec):
        g = np.random.default_rng(2000 + seed)
        hi = max(1, n - 1) if n > 2 else n  # (n > 2: the last label stays unused)
        lab = g.integers(0, hi, size=(h, w))
        if seed != len(spec) - 1:
            coarse = g.integers(0, hi, size=((h + 5) // 6, (w + 5) // 6))
            big = np.kron(coarse, np.ones((6, 6), dtype=np.int64))[:h, :w]
            lab = np.where(g.random((h, w)) < 0.7, big, lab)
        lab = lab.astype(np.int32)
        lab[g.random((h, w)) > density] = -1
        out.append((f"rand{seed}_{h}x{w}_n{n}_d{d}", lab, n, d))
    return out


RANDOM_MAPS = random_label_maps()


def random_maps_for(lab, n, seed=0):
    """Centre map, offsets and centres to go with a random label map."""
    g = np.random.default_rng(3000 + seed)
    h, w = lab.shape
    hm = g.random((h, w)).astype(np.float32)
    off = (g.standard_normal((2, h, w)) * 3).astype(np.float32)
    cen = np.stack([g.integers(0, w, size=n), g.integers(0, h, size=n)], axis=1).astype(np.int32)
    return hm, off, cen


@pytest.mark.parametrize("name,lab,n,d", RANDOM_MAPS, ids=[m[0] for m in RANDOM_MAPS])
def test_tables_host_matches_brute_force_dilation(name, lab, n, d):
    ndi = pytest.importorskip("scipy.ndimage")
    from sleap_nn_amd.inference.ops.segmentation_merge import merge_tables_host

    hm, off, cen = random_maps_for(lab, n)
    T, mom, edges, ridge = merge_tables_host(lab, hm, off, cen, n, 2, d)
    masks = [lab == k for k in range(n)]
    grown = [ndi.binary_dilation(m, iterations=d) if m.any() else m for m in masks]
    for a in range(n):
        for b in range(n):
            assert T[a, b] == (0 if a == b else int((grown[a] & masks[b]).sum())), (name, a, b)
    want = [(i, j) for i in range(n) for j in range(i + 1, n) if T[i, j] + T[j, i] > 0]
    assert [tuple(e[:2]) for e in edges.tolist()] == want and np.array_equal(edges[:, 2], [T[i, j] for i, j in want]) and np.array_equal(edges[:, 3], [T[j, i] for i, j in want])
    t = np.linspace(0.0, 1.0, 48)[7:40]
    for (i, j), r in list(zip(want, ridge))[:50]:  # the reference's own sampling, in floating point
        xi = np.clip(np.round(cen[i][0] + (cen[j][0] - cen[i][0]) * t).astype(int), 0, lab.shape[1] - 1)
        yi = np.clip(np.round(cen[i][1] + (cen[j][1] - cen[i][1]) * t).astype(int), 0, lab.shape[0] - 1)
        assert r == hm[yi, xi].min()
    for k in range(n):
        ys, xs = np.nonzero(masks[k])
        if not len(ys):
            assert not mom[k].any()
            continue
        px = xs * 2.0 + 1.0 + off[0][ys, xs].astype(np.float64)
        py = ys * 2.0 + 1.0 + off[1][ys, xs].astype(np.float64)
        N = len(ys)
        assert abs(cen[k][0] * 2.0 + 1.0 + mom[k][0] / N - px.mean()) <= 1e-9 and abs(cen[k][1] * 2.0 + 1.0 + mom[k][1] / N - py.mean()) <= 1e-9
        assert abs(np.sqrt(max(0.0, mom[k][2] / N - (mom[k][0] / N) ** 2)) - px.std()) <= 1e-6 * max(1.0, px.std())


def test_agglomerations_on_hand_made_edges():
    from sleap_nn_amd.inference.ops.segmentation_merge import agglomerate

    # empty graph, one node, method "none"
    assert agglomerate(3, [], "greedy") == [[0], [1], [2]] and agglomerate(1, [], "multicut") == [[0]] and agglomerate(0, [], "greedy") == []
    assert agglomerate(3, [(0, 1, 0.99)], "none") == [[0], [1], [2]]
    # tie order: the first edge in edge-list order wins; with (0.5,) the merged pair's mean to node 2 is (0.7 + 0.1) / 2 = 0.4: it stays out
    tr = []
    assert agglomerate(3, [(0, 1, 0.7), (0, 2, 0.7), (1, 2, 0.1)], "greedy", thresholds=(0.5,), trace=tr) == [[0, 1], [2]]
    assert tr[0][:2] == (0.7, 0.7) and tr[0][3] is True and tr[-1][3] is False and abs(tr[-1][0] - 0.4) < 1e-12
    assert agglomerate(3, [(0, 2, 0.7), (0, 1, 0.7), (1, 2, 0.1)], "greedy", thresholds=(0.5,)) == [[0, 2], [1]]
    # transitive chain: 0-1 and 1-2 join 0 and 2 although they share no edge; 3 stays alone below the last threshold
    assert agglomerate(4, [(0, 1, 0.9), (1, 2, 0.65), (2, 3, 0.39)], "greedy") == [[0, 1, 2], [3]]
    assert agglomerate(4, [(0, 1, 0.9), (1, 2, 0.65), (2, 3, 0.39)], "multicut") == [[0, 1, 2], [3]]
    # greedy averages parallel edges, multicut adds their costs: mean 0.425 >= 0.4 joins, logit(0.55) + logit(0.3) < 0 does not
    e = [(0, 1, 0.9), (0, 2, 0.55), (1, 2, 0.3)]
    assert agglomerate(3, e, "greedy") == [[0, 1, 2]] and agglomerate(3, e, "multicut") == [[0, 1], [2]]
    # the boundaries themselves: greedy contracts at >= the threshold, multicut only above cost 0
    assert agglomerate(2, [(0, 1, 0.4)], "greedy") == [[0, 1]] and agglomerate(2, [(0, 1, 0.5)], "multicut") == [[0], [1]]
    assert agglomerate(2, [(0, 1, 0.45)], "multicut", join_bias=0.4) == [[0, 1]]
    # groups come ordered by their smallest member
    assert agglomerate(5, [(3, 4, 0.9), (0, 2, 0.9)], "greedy") == [[0, 2], [1], [3, 4]]
    with pytest.raises(ValueError, match="merge method"):
        agglomerate(2, [(0, 1, 0.9)], "watershed")


def test_representative_counts_and_members_after_a_merge():
    from sleap_nn_amd.inference.ops.segmentation_merge import merge_frame

    lab = np.array([[0, 0, 1, 1, -1, 2], [0, 0, 1, 1, -1, 2]], dtype=np.int8)
    cen = np.array([[0, 0], [3, 0], [5, 1], [4, 0]], dtype=np.int32)  # the last centre has no pixels
    sc = np.array([0.5, 0.8, 0.8, 0.9], dtype=np.float32)
    cnt = np.array([4, 4, 2, 0], dtype=np.int32)
    edges = np.array([[0, 1, 2, 2]])
    mom = np.zeros((4, 4))
    new, c, s, n, members = merge_frame(lab, cen, sc, cnt, edges, np.array([1.0], np.float32), mom, 2, method="greedy", w_valley=0.0, w_offset=0.0)
    assert members == [[0, 1], [2], [3]] and n.tolist() == [8, 2, 0] and new.dtype == np.int8
    assert np.array_equal(new, [[0, 0, 0, 0, -1, 1], [0, 0, 0, 0, -1, 1]])
    assert c.tolist() == [[3, 0], [5, 1], [4, 0]] and s.tolist() == [np.float32(0.8), np.float32(0.8), np.float32(0.9)]  # the higher score represents


def _raw(prefix):
    return {"SegmentationHead": torch.from_numpy(MG[f"{prefix}/fg"])[None, None], "InstanceCenterHead": torch.from_numpy(MG[f"{prefix}/hm"])[None, None],
            "CenterOffsetHead": torch.from_numpy(MG[f"{prefix}/off"])[None]}


@pytest.mark.parametrize("name", LAYER_NAMES)
def test_layer_applies_the_area_floor_to_the_merged_mask(name):
    from sleap_nn_amd.inference.layers import MergeSegmentationLayer
    from sleap_nn_amd.inference.preprocess_info import PreprocInfo

    orig, proc, eff, iscale, stride = json.loads(str(MG["layer/info"]))
    area, res, method = name.split("/")
    layer = MergeSegmentationLayer(StubBackend(), stride, min_mask_area=int(area[1:]), full_res_masks=res == "full", merge_method=method)
    assert layer.merge_fragments is True
    info = PreprocInfo(original_size=tuple(orig), processed_size=tuple(proc), eff_scale=torch.tensor([eff], dtype=torch.float32), input_scale=iscale, output_stride=stride)
    got = layer.postprocess(_raw("layer"), info).pred_masks[0]
    assert len(got) == int(MG[f"layer/{name}/n"])
    for i, d in enumerate(got):
        ref_mask, meta = MG[f"layer/{name}/{i}/mask"], MG[f"layer/{name}/{i}/meta"]
        assert d["mask"].dtype == bool and d["mask"].shape == ref_mask.shape and np.array_equal(d["mask"], ref_mask), (name, i)
        assert abs(d["score"] - meta[0]) <= 1e-6
        assert tuple(d["scale"]) == (meta[1], meta[2]) and tuple(d["offset"]) == (meta[3], meta[4])
    if int(area[1:]):  # two fragments fall under the floor alone and pass it merged
        plain = MergeSegmentationLayer(StubBackend(), stride, min_mask_area=int(area[1:]), full_res_masks=res == "full", merge_fragments=False)
        assert len(plain.postprocess(_raw("layer"), info).pred_masks[0]) == len(got) - 1


class RecordedBackend(StubBackend):
    """Returns the head maps handed to it."""

    def __init__(self, raw):
        super().__init__()
        self.raw = raw

    def __call__(self, x):
        return self.raw


def test_layer_reproduces_the_run_directory_from_recorded_head_maps():
    """The ``rundir/...`` case through ``MergeSegmentationLayer`` over a stub backend that returns the reference network's recorded head maps.  The generator
    asserted an empty uncertain set and all merge margins on these frames, and at least one merge: no pixel is excused."""
    from sleap_nn_amd.inference.layers import MergeSegmentationLayer, PostprocessConfig, PreprocessConfig

    rp = json.loads(str(MG["rundir/params"]))
    raw = {"SegmentationHead": torch.from_numpy(MG["rundir/fg"]), "InstanceCenterHead": torch.from_numpy(MG["rundir/hm"]), "CenterOffsetHead": torch.from_numpy(MG["rundir/off"])}
    layer = MergeSegmentationLayer(RecordedBackend(raw), 2, max_stride=8, merge_thresholds=tuple(rp["merge_thresholds"]),
                                   preprocess_config=PreprocessConfig(ensure_grayscale=True), postprocess_config=PostprocessConfig(peak_threshold=rp["peak_threshold"]))
    x, info = layer.preprocess(torch.from_numpy(MG["rundir/frames"]))
    check_rundir(layer.postprocess(layer.backend(x), info).pred_masks)


def check_rundir(got):
    assert len(got) == 2
    for b in range(2):
        ref_masks, ref_scores, ref_scales = MG[f"rundir/{b}/masks"], MG[f"rundir/{b}/scores"], MG[f"rundir/{b}/scales"]
        assert len(got[b]) == int(MG[f"rundir/{b}/n"]) >= 2
        for i, d in enumerate(got[b]):
            assert abs(d["score"] - ref_scores[i]) <= 1e-4, (b, i, d["score"], ref_scores[i])
            assert tuple(d["scale"]) == tuple(ref_scales[i]) and d["mask"].shape == ref_masks[i].shape
            assert np.array_equal(d["mask"], ref_masks[i]), (b, i, int((d["mask"] != ref_masks[i]).sum()))


def test_refusals():
    from sleap_nn_amd import _lib as L
    from sleap_nn_amd.inference.layers import CleanupSegmentationLayer, MergeSegmentationLayer, SegmentationLayer
    from sleap_nn_amd.inference.ops.segmentation import group_enqueue, group_instances_from_offsets

    with pytest.raises(NotImplementedError, match="merge_fragments.*mask_cleanup"):
        MergeSegmentationLayer(StubBackend(), 2, mask_cleanup=True)
    for knob, value in (("mask_cleanup_radius", 2), ("mask_output", "polygon")):
        with pytest.raises(NotImplementedError, match=knob):
            MergeSegmentationLayer(StubBackend(), 2, **{knob: value})
    for cls in (SegmentationLayer, CleanupSegmentationLayer):  # the other layers keep refusing the knob
        with pytest.raises(NotImplementedError, match="merge_fragments"):
            cls(StubBackend(), 2, merge_fragments=True)
    with pytest.raises(ValueError, match="merge method"):
        MergeSegmentationLayer(StubBackend(), 2, merge_method="watershed")
    (fg, hm, off), p = case("ridge_vs_valley")
    with pytest.raises(ValueError, match="merge method"):
        group_instances_from_offsets(fg, hm, off, merge_fragments=True, merge_method="watershed")
    with pytest.raises(NotImplementedError, match="merge_fragments.*mask_cleanup"):
        group_instances_from_offsets(fg, hm, off, merge_fragments=True, mask_cleanup=True)
    # merge_dilate = 5: the device path's argument check names the knob (before it touches a tensor), and the C entry point rejects d = 5 before any launch
    with pytest.raises(ValueError, match="merge_dilate"):
        group_enqueue(fg, hm, off, 0.5, 0.2, 2, None, 3, None, 3, merge_fragments=True, merge_dilate=5)
    with pytest.raises(ValueError, match="merge_dilate"):
        group_instances_from_offsets(fg, hm, off, device="cuda:0", merge_fragments=True, merge_dilate=5)
    assert group_instances_from_offsets(fg, hm, off, merge_fragments=True, merge_dilate=5).members[0] == [[0, 2], [1], [3], [4]]  # (the host path dilates as far as asked)
    lib, q = L.lib(), C.c_void_p(4096)  # (never dereferenced: every call below is rejected by the argument checks)
    args = lambda d=1, mc=8, lb=1, sb=1 << 20, sp=q, first=q: (first, q, q, 1, 4, 4, 2, d, q, q, mc, lb, q, q, q, 4, sp, sb, None)
    assert lib.ph_seg_merge_tables(*args(d=5)) == L.PH_E_INVALID and "dilate" in lib.ph_last_error().decode()
    assert lib.ph_seg_merge_tables(*args(d=0)) == L.PH_E_INVALID
    assert lib.ph_seg_merge_tables(*args(first=None)) == L.PH_E_INVALID
    assert lib.ph_seg_merge_tables(*args(mc=200, lb=1)) == L.PH_E_INVALID  # 200 centres in one-byte labels
    assert lib.ph_seg_merge_tables(*args(mc=5000, lb=4)) == L.PH_E_INVALID  # beyond the dense table
    assert lib.ph_seg_merge_tables(*args(sp=C.c_void_p(4100))) == L.PH_E_INVALID  # unaligned scratch
    assert lib.ph_seg_merge_tables(*args(sb=8)) == L.PH_E_INVALID  # short scratch


@pytest.mark.parametrize("seg_kw,cls_name", [({"merge_fragments": True, "merge_method": "multicut", "merge_dilate": 2, "merge_thresholds": (0.7, 0.5)}, "MergeSegmentationLayer"),
                                             ({"merge_fragments": False}, "SegmentationLayer"), ({"mask_cleanup": True}, "CleanupSegmentationLayer")])
def test_select_layer_routes_on_the_knob(seg_kw, cls_name, monkeypatch):
    from sleap_nn_amd.inference import predictor as P
    from sleap_nn_amd.inference.layers import PostprocessConfig
    from sleap_nn_amd.inference.loaders import load_model_assets

    a = load_model_assets(os.path.join(G.GOLDEN_DIR, "ckpt_dirs", "tiny_bottomup_segmentation"))
    monkeypatch.setattr(P, "HipBackend", lambda model, device: StubBackend(model))
    layer = P._select_layer([a], "cuda:0", PostprocessConfig(peak_threshold=0.2), 5, seg_kw=dict(seg_kw, min_mask_area=7))
    assert type(layer).__name__ == cls_name and layer.merge_fragments is bool(seg_kw.get("merge_fragments")) and layer.min_mask_area == 7 and layer.max_instances == 5
    if seg_kw.get("merge_fragments"):
        assert (layer.merge_method, layer.merge_dilate, layer.merge_thresholds, layer.merge_w_valley, layer.merge_w_offset) == ("multicut", 2, (0.7, 0.5), 1.0, 0.25)
        with pytest.raises(NotImplementedError, match="mask_cleanup"):
            P._select_layer([a], "cuda:0", PostprocessConfig(), None, seg_kw={"merge_fragments": True, "mask_cleanup": True})
    import inspect

    sig = inspect.signature(P.Predictor.from_model_paths).parameters  # the reference's defaults
    assert [sig[k].default for k in ("merge_method", "merge_thresholds", "merge_w_valley", "merge_w_offset", "merge_dilate")] == ["greedy", (0.85, 0.6, 0.4), 1.0, 0.25, 1]


@pytest.mark.parametrize("name", PLAIN_NAMES)
def test_merge_off_is_the_recorded_unmerged_result(name):
    from sleap_nn_amd.inference.ops.segmentation import group_instances_from_offsets

    (fg, hm, off), p = plain_case(name)
    g = group_instances_from_offsets(fg, hm, off, merge_fragments=False, **group_kwargs(p))
    assert g.members is None and g.holes is None
    check_grouping(name, g, p)


def test_abi_declares_the_merge_entry_points():
    import re

    from sleap_nn_amd import _lib as L

    header = open(os.path.join(os.path.dirname(G.GOLDEN_DIR), "..", "include", "posehip.h")).read()
    assert int(re.search(r"^#define\s+PH_VERSION\s+(\d+)", header, re.M).group(1)) >= 116
    assert {"ph_seg_merge_tables", "ph_seg_merge_scratch_bytes"} <= set(L.SIGNATURES)
    lib = L.lib()
    assert lib.ph_seg_merge_scratch_bytes(0, 4, 4, 8) == 0 and lib.ph_seg_merge_scratch_bytes(1, 4, 4, 5000) == 0
    assert lib.ph_seg_merge_scratch_bytes(2, 4, 4, 8) >= 2 * (8 * 8 + 8 * 4) * 4
