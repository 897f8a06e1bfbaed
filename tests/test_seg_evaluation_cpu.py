"""Mask evaluation on the host (``sleap_nn_amd/evaluation.py``: ``mask_pair_stats``, ``match_masks``, ``mask_boundary`` / ``boundary_iou``, ``MaskEvaluator``,
``SemanticEvaluator``, ``EpochEndMaskEvaluator``) against the reference's recorded results (``tests/golden/seg_evaluation.npz``, written by
tools/gen_seg_evaluation_golden.py; boundary numbers are the reference's code over a NumPy / SciPy stand-in for OpenCV's ``erode``).

Bars: intersections, areas, match indices, counts, the ``per_size`` tables, the ``mask_voc.*`` arrays, boundary masks and NaN positions are equal; IoUs and
the scalar metrics agree to 1e-12 relative (the same float64 operations on the same integers; the slack is for summation order only)."""
import numpy as np
import pytest

from tests import _golden as G

RTOL = 1e-12
PAIR_CASES = ["a", "b1", "b2", "c", "d"]
MATCH_KEYS = ("matched_pred", "matched_gt", "unmatched_pred", "unmatched_gt", "matched_ious")
_cache = {}


def Z():
    if "z" not in _cache:
        _cache["z"] = G.load("seg_evaluation.npz")
    return _cache["z"]


def unpack(bits, shape):
    shape = tuple(int(v) for v in shape)
    return np.unpackbits(bits, count=int(np.prod(shape))).reshape(shape).astype(bool)


def pair_case(name):
    """Inputs of a recorded pair-statistics case: ``pred`` (B, P, ph, pw) bool, ``labels`` (B, ph, pw) int8, ``gt`` (B, G, H, W) bool, counts, stride."""
    if ("pair", name) not in _cache:
        z, k = Z(), f"pair/{name}/"
        _cache[("pair", name)] = dict(pred=unpack(z[k + "pred_bits"], z[k + "pred_shape"]), gt=unpack(z[k + "gt_bits"], z[k + "gt_shape"]), labels=z[k + "labels"],
                                      n_pred=z[k + "n_pred"], n_gt=z[k + "n_gt"], s=int(z[k + "stride"]))
    return _cache[("pair", name)]


def ev_case():
    if "ev" not in _cache:
        z = Z()
        _cache["ev"] = dict(labels=z["ev/labels"], gt=unpack(z["ev/gt_bits"], z["ev/gt_shape"]), n_pred=z["ev/n_pred"], n_gt=z["ev/n_gt"], scores=z["ev/scores"],
                            s=int(z["ev/stride"]))
    return _cache["ev"]


def boundary_case(name):
    z, k = Z(), f"boundary/{name}/"
    return unpack(z[k + "mask_bits"], z[k + "shape"]), int(z[k + "d"]), unpack(z[k + "out_bits"], z[k + "shape"])


def check_tables(name, form, inter, pa, ga):
    """Padded integer tables against the recorded ones (which are 0 in the padding)."""
    z, k = Z(), f"pair/{name}/{form}/"
    for got, key in ((inter, "inter"), (pa, "pred_area"), (ga, "gt_area")):
        got = np.asarray(got)
        assert got.dtype.kind == "i" and got.shape == z[k + key].shape and np.array_equal(got, z[k + key]), (name, form, key)


def check_frames(name, form, stats):
    """``mask_pair_stats`` + ``match_masks`` per frame against the recorded results."""
    from sleap_nn_amd.evaluation import match_masks

    z, k, c = Z(), f"pair/{name}/{form}/", pair_case(name)
    want = {m: G.ragged(z, k + m) for m in MATCH_KEYS}
    for b, (iou, inter, pa, ga) in enumerate(stats):
        n_p, n_g = int(c["n_pred"][b]), int(c["n_gt"][b])
        assert iou.shape == (n_p, n_g) and iou.dtype == np.float64
        assert np.array_equal(inter, z[k + "inter"][b, :n_p, :n_g]) and np.array_equal(pa, z[k + "pred_area"][b, :n_p]) and np.array_equal(ga, z[k + "gt_area"][b, :n_g])
        np.testing.assert_allclose(iou, z[k + "iou"][b, :n_p, :n_g], rtol=RTOL, atol=0)
        got = match_masks(iou, 0.5)
        for j, m in enumerate(MATCH_KEYS[:4]):
            assert np.array_equal(got[j], want[m][b]), (name, form, b, m)
        np.testing.assert_allclose(got[4], want["matched_ious"][b], rtol=RTOL, atol=0)


def matched_pairs(name, form):
    """The matched (prediction, ground truth) masks of a case on the image grid, and their recorded boundary IoUs."""
    z, k, c = Z(), f"pair/{name}/{form}/", pair_case(name)
    mp, mg = G.ragged(z, k + "matched_pred"), G.ragged(z, k + "matched_gt")
    pm, gm = [], []
    for b in range(len(mp)):
        for p, g in zip(mp[b], mg[b]):
            cell = c["pred"][b, p] if form == "stack" else c["labels"][b] == p
            pm.append(np.repeat(np.repeat(cell, c["s"], axis=0), c["s"], axis=1))
            gm.append(c["gt"][b, g])
    return np.stack(pm), np.stack(gm), z[k + "boundary_iou_cat"]


def flatten(d, prefix=""):
    out = {}
    for k, v in d.items():
        if isinstance(v, dict):
            out.update(flatten(v, f"{prefix}{k}/"))
        else:
            out[prefix + k] = v
    return out


def check_dict(got, prefix, exact=()):
    """A metrics dictionary against the recorded one: same keys, strings and integers equal, NaN in the same places, floats to RTOL -- or equal under ``exact``."""
    z = Z()
    got = flatten(got)
    want = {k[len(prefix):]: z[k] for k in z.files if k.startswith(prefix)}
    assert set(got) == set(want), set(got) ^ set(want)
    for k, w in want.items():
        v = np.asarray(got[k])
        if w.dtype.kind in "US":
            assert str(v) == str(w), k
            continue
        assert v.shape == w.shape, k
        if w.dtype.kind in "iub":
            assert v.dtype.kind in "iub" and np.array_equal(v, w), k
            continue
        assert np.array_equal(np.isnan(v.astype(float)), np.isnan(w)), k
        if any(k.startswith(e) for e in exact):
            assert np.array_equal(v.astype(float), w, equal_nan=True), k
        else:
            np.testing.assert_allclose(v.astype(float), w, rtol=RTOL, atol=0, equal_nan=True, err_msg=k)


def feed_mask_evaluator(ev, to=lambda a: a, form="label"):
    """The 12 recorded frames in three batches of four."""
    c = ev_case()
    for b0 in range(0, len(c["n_pred"]), 4):
        sl = slice(b0, b0 + 4)
        if form == "label":
            pred = to(c["labels"][sl])
        else:
            pred = to(np.ascontiguousarray((c["labels"][sl, None] == np.arange(c["scores"].shape[1], dtype=np.int8)[None, :, None, None])))
        ev.add_batch(pred, c["scores"][sl], to(c["gt"][sl]), c["n_pred"][sl], c["n_gt"][sl], c["s"])
    return ev


def feed_semantic_evaluator(ev, to=lambda a: a):
    c = ev_case()
    gt_fg = c["gt"].any(axis=1)
    for b0 in range(0, len(c["n_pred"]), 4):
        ev.add_batch(to(c["labels"][b0 : b0 + 4] >= 0), to(gt_fg[b0 : b0 + 4]), c["s"])
    return ev


# ---- tests ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("form", ["stack", "label"])
@pytest.mark.parametrize("name", PAIR_CASES)
def test_pair_stats_and_matching(name, form):
    from sleap_nn_amd.evaluation import mask_pair_stats, mask_pair_tables

    c = pair_case(name)
    pred = c["pred"] if form == "stack" else c["labels"]
    check_tables(name, form, *mask_pair_tables(pred, c["gt"], c["n_pred"], c["n_gt"], c["s"]))
    check_frames(name, form, mask_pair_stats(pred, c["gt"], c["n_pred"], c["n_gt"], c["s"]))


def test_cpu_tensors_take_the_host_path():
    import torch

    from sleap_nn_amd.evaluation import mask_pair_stats

    c = pair_case("b1")
    check_frames("b1", "label", mask_pair_stats(torch.from_numpy(c["labels"]).to(torch.int16), torch.from_numpy(c["gt"]), c["n_pred"], c["n_gt"], c["s"]))


def test_empty_union_is_one_and_empty_sets_match_nothing():
    from sleap_nn_amd.evaluation import match_masks

    z = Z()
    assert z["pair/a/stack/iou"][0, 2, 3] == 1.0 and z["pair/a/stack/inter"][0, 2, 3] == 0  # an empty prediction against an empty ground-truth mask
    for shape, up, ug in (((0, 0), 0, 0), ((0, 3), 0, 3), ((2, 0), 2, 0)):
        mp, mg, unp, ung, mi = match_masks(np.zeros(shape))
        assert len(mp) == len(mg) == len(mi) == 0 and np.array_equal(unp, np.arange(up)) and np.array_equal(ung, np.arange(ug))


@pytest.mark.parametrize("name", ["a", "d", "d_wide"])
def test_boundary_masks(name):
    from sleap_nn_amd.evaluation import boundary_width, mask_boundary

    masks, d, want = boundary_case(name)
    if name != "d_wide":
        assert boundary_width(*masks.shape[1:]) == d
    got = mask_boundary(masks, d)
    assert got.dtype == bool and np.array_equal(got, want)
    if name == "d_wide":  # d = 18 is wider than every blob but the large one: their boundary is the mask itself
        assert sum(bool(np.array_equal(want[k], masks[k])) for k in range(len(masks))) >= len(masks) - 1


@pytest.mark.parametrize("name", ["a", "b1", "b2", "d"])
def test_boundary_iou_of_matched_pairs(name):
    from sleap_nn_amd.evaluation import boundary_iou

    pm, gm, want = matched_pairs(name, "stack")
    assert len(want) > 0
    np.testing.assert_allclose(boundary_iou(pm, gm), want, rtol=RTOL, atol=0)


@pytest.mark.parametrize("P,G", [(65, 3), (4, 65), (70, 66)])
def test_beyond_the_device_cap(P, G):
    """More than 64 masks on a side: the host path, against a brute-force count."""
    from sleap_nn_amd.evaluation import MAX_DEVICE_MASKS, mask_pair_stats

    assert MAX_DEVICE_MASKS == 64
    g = np.random.default_rng(P * 100 + G)
    pred, gt = g.random((2, P, 9, 11)) > 0.7, g.random((2, G, 20, 19)) > 0.6
    n_pred, n_gt = [P, P - 2], [G - 1, G]
    up = np.zeros((2, P, 20, 22), bool)
    up[:, :, :18] = np.repeat(np.repeat(pred, 2, axis=2), 2, axis=3)
    gc = np.zeros((2, G, 20, 22), bool)
    gc[..., :19] = gt
    for b, (iou, inter, pa, ga) in enumerate(mask_pair_stats(pred, gt, n_pred, n_gt, 2)):
        want = (up[b, : n_pred[b], None] & gc[b, None, : n_gt[b]]).sum(axis=(2, 3))
        union = (up[b, : n_pred[b], None] | gc[b, None, : n_gt[b]]).sum(axis=(2, 3))
        assert np.array_equal(inter, want) and np.array_equal(pa, up[b, : n_pred[b]].sum(axis=(1, 2))) and np.array_equal(ga, gc[b, : n_gt[b]].sum(axis=(1, 2)))
        np.testing.assert_allclose(iou, want / union, rtol=RTOL, atol=0)


@pytest.mark.parametrize("form", ["label", "stack"])
def test_mask_evaluator(form):
    from sleap_nn_amd.evaluation import MaskEvaluator

    ev = feed_mask_evaluator(MaskEvaluator(0.5), form=form)
    mm = ev.mask_metrics()
    check_dict(mm, "ev/mask_metrics/", exact=("per_size/",))
    check_dict(ev.mask_voc_metrics(), "ev/mask_voc_metrics/", exact=("mask_voc.",))
    assert mm["oversegmentation"] >= 1 and mm["undersegmentation"] >= 1 and np.isnan(mm["mean_cldice"])
    assert all(set(f) == {"iou", "inter", "gt_areas", "pred_areas", "pred_scores"} and all(v.ndim <= 2 for v in f.values()) for f in ev._frames)  # no masks are kept


def test_semantic_evaluator():
    from sleap_nn_amd.evaluation import SemanticEvaluator

    sm = feed_semantic_evaluator(SemanticEvaluator()).semantic_metrics()
    check_dict(sm, "ev/semantic_metrics/")
    assert sm["n_frames"] == 11 and np.isnan(sm["cldices"]).all()  # the frame without ground truth is skipped


def test_epoch_end_mask_evaluator_frequency_and_reset():
    from sleap_nn_amd.evaluation import EpochEndMaskEvaluator

    e = EpochEndMaskEvaluator(eval_frequency=2)
    assert e.compute(1) is None  # nothing added
    feed_mask_evaluator(e)
    assert not e.due(0) and e.compute(0) is None  # off frequency: dropped
    assert e.compute(1) is None  # ... and reset
    feed_mask_evaluator(e)
    out = e.compute(1)
    assert set(out) == {"mask_metrics", "mask_voc_metrics"}
    check_dict(out["mask_metrics"], "ev/mask_metrics/", exact=("per_size/",))
    assert e.compute(3) is None
    s = EpochEndMaskEvaluator(semantic=True)
    feed_semantic_evaluator(s)
    check_dict(s.compute(0)["semantic_metrics"], "ev/semantic_metrics/")
