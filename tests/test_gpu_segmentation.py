"""Segmentation on the GPU: the grouping kernels through the C ABI against the reference's recorded results (label map, centres and
counts identical, scores to 1e-6), the semantic kernel, the model goldens (1e-4, the project's standing bound) and a run directory
through ``Predictor``.  Goldens: tools/gen_segmentation_golden.py."""
import json
import os

import numpy as np
import pytest
import torch

from tests import _golden as G
from tests.test_segmentation_cpu import GROUP_NAMES, LAYER_INFOS, SEG, _case, check_grouping, group_kwargs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CMS_ATOL = 1e-4


def _group(name, **kw):
    from sleap_nn_amd.inference.ops.segmentation import group_instances_from_offsets

    (fg, hm, off), p = _case(name)
    return group_instances_from_offsets(fg.to(DEV), hm.to(DEV), off.to(DEV), **group_kwargs(p), **kw), p


@pytest.mark.parametrize("name", GROUP_NAMES)
def test_grouping_matches_reference(name):
    """Default capacities: 'lattice' (2 304 centres) comes back twice -- for a candidate list beyond the LDS one, then for two-byte labels."""
    g, p = _group(name)
    check_grouping(name, g, p)
    n = max(len(c) for c in g.centers)
    assert g.labels.dtype == (np.int8 if n <= 127 else np.int16)


def test_retry_on_small_capacities():
    g, p = _group("many_96x96", cap=16, max_centers=8)
    check_grouping("many_96x96", g, p)
    g, p = _group("max_instances", cap=70, max_centers=4)
    check_grouping("max_instances", g, p)


@pytest.mark.parametrize("name", ["many_96x96", "gate", "batch3"])
def test_non_default_stream_and_repeatable(name):
    g0, p = _group(name)
    s = torch.cuda.Stream(DEV)
    with torch.cuda.stream(s):
        g1, _ = _group(name)
    g2, _ = _group(name)
    check_grouping(name, g1, p)
    for a, b in ((g0, g1), (g0, g2)):
        assert np.array_equal(a.labels, b.labels)
        for k in range(len(a.centers)):
            assert np.array_equal(a.centers[k], b.centers[k]) and np.array_equal(a.scores[k], b.scores[k]) and np.array_equal(a.counts[k], b.counts[k])


def test_c_abi_rejects_bad_arguments():
    import ctypes as C

    from sleap_nn_amd import _lib as L

    t = torch.zeros(64, dtype=torch.int32, device=DEV)
    p = C.c_void_p(t.data_ptr())
    assert L.lib().ph_seg_center_peaks(p, 1, 4, 4, 0.2, 4, 0, 16, 8, p, p, p, p, 1, p, 1 << 20, None) == L.PH_E_INVALID  # even window
    assert L.lib().ph_seg_assign(p, p, 1, 4, 4, 0.5, 2, p, p, 200, 1, p, None, p, None) == L.PH_E_INVALID  # 200 centres in one-byte labels
    assert L.lib().ph_seg_center_peaks(p, 1, 4, 4, 0.2, 3, 0, 16, 8, p, p, p, p, 1, p, 8, None) == L.PH_E_WORKSPACE


@pytest.mark.parametrize("iname", sorted(LAYER_INFOS))
def test_semantic_kernel(iname):
    from sleap_nn_amd.inference.ops.segmentation import semantic_masks

    fg = torch.from_numpy(SEG[f"layer/{iname}/fg"])
    batch = torch.stack([fg, torch.full_like(fg, 0.1), fg.flip(0)])[:, None]  # (the middle frame has no foreground)
    masks, counts, scores = semantic_masks(batch.to(DEV), 0.5)
    assert np.array_equal(masks, (batch[:, 0] > 0.5).numpy())
    rec = SEG[f"layer/{iname}/a0/stride/sem/0/mask"]  # the reference's mask of this map, cropped to its valid extent
    assert np.array_equal(masks[0][: rec.shape[0], : rec.shape[1]], rec)
    assert counts.tolist() == [int(m.sum()) for m in masks] and counts[1] == 0 and scores[1] == 0.0
    ref = SEG[f"layer/{iname}/a0/stride/sem/0/meta"][0]  # the reference's score of this map: mean probability over the mask
    for b in (0, 2):
        print(iname, b, "score", scores[b], "reference", ref, "relative error", abs(scores[b] - ref) / ref)
        assert abs(scores[b] - ref) <= 1e-5 * ref  # (the summation order differs: that is the whole allowance)
    again = semantic_masks(batch.to(DEV), 0.5)
    assert np.array_equal(again[0], masks) and np.array_equal(again[2], scores)


@pytest.mark.parametrize("prefix", ["bu", "sem"])
@pytest.mark.parametrize("program", ["default", "conv_precision_0", "unfused"])
def test_model_goldens(prefix, program):
    from sleap_nn_amd.architectures.model import Model

    z = G.load("unet_tiny_seg.npz")
    cfg = json.loads(str(z[f"{prefix}/config_json"]))
    m = Model("unet", cfg["backbone"], cfg["heads"], cfg["model_type"])
    m.load_state_dict({k[len(prefix) + 3 :]: torch.from_numpy(z[k]) for k in z.files if k.startswith(f"{prefix}/w/")}, strict=True)
    m.to(DEV)
    if program == "conv_precision_0":
        m.set_option("conv_precision", 0)
    elif program == "unfused":
        m.set_fusion(False)
    out = m(torch.from_numpy(z[f"{prefix}/image"]).squeeze(1).to(DEV))
    torch.cuda.synchronize()
    keys = [k for k in z.files if k.startswith(f"{prefix}/out/")]
    assert len(keys) == (3 if prefix == "bu" else 1)
    for k in keys:
        ref = torch.from_numpy(z[k])
        got = out[k.split("/")[-1]].cpu()
        assert got.shape == ref.shape
        err = (got - ref).abs().max().item()
        print(prefix, program, k, "max abs error", err)
        assert err <= CMS_ATOL, (k, err)
    fg = out["SegmentationHead"]
    assert float(fg.min()) >= 0.0 and float(fg.max()) <= 1.0  # probabilities: the sigmoid is the head op's epilogue


def test_backward_is_refused():
    import ctypes as C

    from sleap_nn_amd import _lib as L
    from sleap_nn_amd.architectures.model import Model

    z = G.load("unet_tiny_seg.npz")
    cfg = json.loads(str(z["sem/config_json"]))
    m = Model("unet", cfg["backbone"], cfg["heads"], cfg["model_type"]).train(True).to(DEV)
    x = torch.from_numpy(z["sem/image"]).squeeze(1).to(DEV)
    out = m(x)
    t = torch.zeros(1 << 16, dtype=torch.float32, device=DEV)
    p = C.c_void_p(t.data_ptr())
    ptrs = (C.c_void_p * 1)(out["SegmentationHead"].data_ptr())
    lw = (C.c_float * 1)(1.0)
    rc = L.lib().ph_model_backward(m._handle, C.c_void_p(x.data_ptr()), 0, x.shape[0], 1, x.shape[2], x.shape[3], C.c_void_p(m._workspace.data_ptr()), p, t.numel() * 4,
                                   ptrs, ptrs, lw, None, 0, 2.0, 2, 0, 5.0, p, p, None)
    assert rc == L.PH_E_INVALID and "segmentation" in L.lib().ph_last_error().decode()


def test_run_directory_through_predictor():
    from sleap_nn_amd.inference.layers import SegmentationLayer
    from sleap_nn_amd.inference.predictor import Predictor

    pred = Predictor.from_model_paths([os.path.join(G.GOLDEN_DIR, "ckpt_dirs", "tiny_bottomup_segmentation")], device=DEV, batch_size=2)
    assert isinstance(pred.layer, SegmentationLayer)
    outs = pred.predict(SEG["rundir/frames"])
    assert len(outs) == 1 and len(outs[0].pred_masks) == 2
    unc = SEG["rundir/uncertain"]
    for b in range(2):
        got = outs[0].pred_masks[b]
        ref_masks, ref_scores, ref_scales = SEG[f"rundir/{b}/masks"], SEG[f"rundir/{b}/scores"], SEG[f"rundir/{b}/scales"]
        assert len(got) == int(SEG[f"rundir/{b}/n"]) >= 2
        skip = unc[b][: ref_masks.shape[1], : ref_masks.shape[2]]
        assert unc[b].mean() <= 0.005  # the recorded uncertain set (reference fg within 1e-3 of the threshold / two nearest centres within 1e-3 relative)
        for i, d in enumerate(got):
            assert abs(d["score"] - ref_scores[i]) <= 1e-4, (b, i, d["score"], ref_scores[i])
            assert tuple(d["scale"]) == tuple(ref_scales[i]) and d["mask"].shape == ref_masks[i].shape
            diff = d["mask"] != ref_masks[i]
            print("frame", b, "instance", i, "pixels that differ (all inside the uncertain set?)", int(diff.sum()), int((diff & ~skip).sum()))
            assert not (diff & ~skip).any(), (b, i, int((diff & ~skip).sum()))


def test_semantic_run_directory_through_predictor():
    from sleap_nn_amd.inference.layers import SemanticSegmentationLayer
    from sleap_nn_amd.inference.predictor import Predictor

    pred = Predictor.from_model_paths([os.path.join(G.GOLDEN_DIR, "ckpt_dirs", "tiny_semantic_segmentation")], device=DEV, batch_size=2, fg_threshold=0.5)
    assert isinstance(pred.layer, SemanticSegmentationLayer)
    out = pred.predict(SEG["rundir/frames"])[0]
    raw = pred.layer.backend(pred.layer.preprocess(torch.from_numpy(SEG["rundir/frames"]))[0])["SegmentationHead"].cpu()
    for b in range(2):
        m = (raw[b, 0] > 0.5).numpy()[:36, :50]  # 72 x 100 frames at stride 2
        if not m.any():
            assert out.pred_masks[b] == []
            continue
        assert len(out.pred_masks[b]) == 1 and np.array_equal(out.pred_masks[b][0]["mask"], m)
        assert out.pred_masks[b][0]["scale"] == (0.5, 0.5)
