"""Cross-frame tracking without a GPU: ``sleap_nn_amd.tracking`` against the reference's recorded runs (tests/golden/tracking.npz, written by
tools/gen_tracking_golden.py from the reference's own ``Tracker``; the sleap-io objects and the mask resample rule there are stand-ins, see that tool).

Every golden case runs three ways: frame by frame through ``Tracker.track`` (NumPy scores), in batches of 3 through ``track_outputs`` with the pair tables
(``ph_track_pose_scores`` for poses) and in batches of 3 without them.  Demanded: ids IDENTICAL to the reference; tracking scores and ``get_scores``' matrices
within 1e-9 (float64 arithmetic of a few hundred operations stays orders of magnitude below that, and the generator refused every case whose ids move when each
score is perturbed by 1e-9 relative, so 1e-9 cannot flip a match); mask scores exactly equal (integer counts, one division).
"""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest
import torch

from tests import _golden as G

Z = G.load("tracking.npz")
PARAMS = json.loads(str(Z["params"]))
POSE_CASES = {n: {k: v for k, v in kw.items() if k != "_seq"} for n, kw in PARAMS["pose_cases"].items()}
POSE_SEQ = {n: kw.get("_seq", "plain") for n, kw in PARAMS["pose_cases"].items()}
MASK_CASES = PARAMS["mask_cases"]
TOL = 1e-9
worst = {"pose": 0.0}


def pose_frames(seq):
    pts, sc, counts = Z[f"seq/{seq}/points"], Z[f"seq/{seq}/scores"], Z[f"seq/{seq}/counts"]
    return [(pts[t, : counts[t]], sc[t, : counts[t]]) for t in range(len(counts))]


def expected(name, t):
    key = f"{name}/scores/{t}"
    return Z[f"{name}/ids/{t}"], Z[f"{name}/tracking_scores/{t}"], (Z[key] if key in Z.files else None)


def close(a, b, tol):
    """Equal where non-finite (NaN with NaN, inf with inf of one sign), within ``tol`` (absolute, and relative for large values) elsewhere; returns the largest
    difference."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    fin = np.isfinite(b)
    assert np.array_equal(np.isfinite(a), fin)
    assert np.array_equal(a[~fin], b[~fin], equal_nan=True)
    d = np.abs(a[fin] - b[fin]) / np.maximum(1.0, np.abs(b[fin]))
    assert d.size == 0 or d.max() <= tol, d.max()
    return float(d.max()) if d.size else 0.0


def check_frame(name, t, tracker, ids, tsc, tol, kind="pose"):
    e_ids, e_tsc, e_sc = expected(name, t)
    assert np.array_equal(ids, e_ids), (name, t, ids, e_ids)
    w = close(tsc, e_tsc, tol)
    assert (tracker.last_scores is None) == (e_sc is None), (name, t)
    if e_sc is not None:
        w = max(w, close(tracker.last_scores, e_sc, tol))
    if kind == "pose":
        worst["pose"] = max(worst["pose"], w)


def pose_outputs(frames, t0, n):
    from sleap_nn_amd.inference.outputs import Outputs

    chunk = frames[t0 : t0 + n]
    I = max(len(p) for p, _s in chunk) + 1  # one NaN-padded slot more than the fullest frame
    kp = torch.full((len(chunk), I, chunk[0][0].shape[1], 2), float("nan"), dtype=torch.float64)
    sc = torch.full((len(chunk), I), float("nan"), dtype=torch.float64)
    valid = torch.zeros((len(chunk), I), dtype=torch.bool)  # (the sparse sequence has an instance without a visible node: NaN rows alone cannot name the padding)
    for b, (p, s) in enumerate(chunk):
        kp[b, : len(p)], sc[b, : len(p)], valid[b, : len(p)] = torch.from_numpy(p), torch.from_numpy(s), True
    return Outputs(pred_keypoints=kp, instance_scores=sc, instance_valid=valid, frame_indices=torch.arange(t0, t0 + len(chunk)))


@pytest.mark.parametrize("name", sorted(POSE_CASES))
def test_pose_case_frame_by_frame(name):
    from sleap_nn_amd.tracking import Tracker

    tr = Tracker.from_config(**POSE_CASES[name])
    for t, (p, s) in enumerate(pose_frames(POSE_SEQ[name])):
        ids, tsc = tr.track(p, t, instance_scores=s)
        assert ids.dtype == np.int64 and tsc.dtype == np.float64 and ids.shape == (len(p),)
        check_frame(name, t, tr, ids, tsc, TOL)
    print(name, "largest |score - reference|:", worst["pose"])


@pytest.mark.parametrize("use_tables", [True, False])
@pytest.mark.parametrize("name", sorted(POSE_CASES))
def test_pose_case_in_batches_of_three(name, use_tables):
    """``track_outputs`` on batches of 3 gives what frame-by-frame ``track`` gives: the reference's ids.  With the tables every pair score inside their reach comes
    from ``ph_track_pose_scores``."""
    from sleap_nn_amd.tracking import Tracker

    tr = Tracker.from_config(**POSE_CASES[name])
    frames = pose_frames(POSE_SEQ[name])
    hits = []
    for t0 in range(0, len(frames), 3):
        o = pose_outputs(frames, t0, 3)
        spy_scores = []
        inner = tr._track_entries

        def spy(*a, _inner=inner, **k):
            r = _inner(*a, **k)
            spy_scores.append(tr.last_scores)
            return r

        tr._track_entries = spy
        out = tr.track_outputs(o, use_tables=use_tables)
        tr._track_entries = inner
        assert out.instance_track_ids.dtype == torch.int64 and tuple(out.instance_track_ids.shape) == tuple(o.pred_keypoints.shape[:2])
        for b in range(o.batch_size):
            n = len(frames[t0 + b][0])
            tr.last_scores = spy_scores[b]
            check_frame(name, t0 + b, tr, out.instance_track_ids[b, :n].numpy(), out.instance_tracking_scores[b, :n].numpy(), TOL)
            assert (out.instance_track_ids[b, n:] == -1).all() and torch.isnan(out.instance_tracking_scores[b, n:]).all()
    if use_tables:
        assert tr.table_hits > 0
        if not tr.is_local_queue:
            assert tr.pair_calls == 0  # the fixed window never looks further back than the tables reach
    else:
        assert tr.table_hits == 0


def test_native_pose_scores_equal_numpy():
    """``ph_track_pose_scores`` against the NumPy functions, every method, with NaN nodes, an instance without a visible node, ragged counts, history in use."""
    from sleap_nn_amd.tracking import scoring as S

    g = np.random.default_rng(3)
    B, L, I, N = 3, 4, 5, 6
    w = 0.0
    for method, n in (("oks", N), ("euclidean_dist", N), ("euclidean_dist", 1), ("cosine_sim", 1), ("iou", 2)):
        cur, hist = g.uniform(0, 100, (B, I, n, 2)), g.uniform(0, 100, (L, I, n, 2))
        if method == "oks":
            cur[g.uniform(size=cur.shape[:3]) < 0.2] = np.nan
            hist[g.uniform(size=hist.shape[:3]) < 0.2] = np.nan
            cur[1, 2] = np.nan
        if method == "iou":
            for a in (cur, hist):
                a[..., 1, :] = a[..., 0, :] + g.uniform(1, 30, a[..., 0, :].shape)
        counts = np.array([5, 3, 4, 0, 5, 2, 5], dtype=np.int32)
        for n_hist in (0, 2, 4):
            out = S.pose_pair_scores(cur, hist, n_hist, counts, method, 0.05)
            for b in range(B):
                for k in range(1, L + 1):
                    src, f = (cur, b - k) if b >= k else (hist, L - (k - b))
                    reach = b >= k or k - b <= n_hist
                    nj = counts[b - k] if b >= k else counts[B + L - (k - b)]
                    for i in range(I):
                        for j in range(I):
                            if not reach or i >= counts[b] or j >= nj:
                                assert np.isnan(out[b, k - 1, i, j])
                                continue
                            a, p = cur[b, i], src[f, j]
                            ref = {"oks": lambda: S.oks_score(a, p, 0.05), "iou": lambda: S.bbox_iou(a.reshape(-1), p.reshape(-1)),
                                   "euclidean_dist": lambda: S.neg_euclidean(a, p), "cosine_sim": lambda: S.cosine_sim(a.reshape(-1), p.reshape(-1))}[method]()
                            w = max(w, close(out[b, k - 1, i, j], ref, TOL))
    print("largest |native - NumPy|:", w)


def test_pose_scores_abi_rejects_bad_arguments():
    from sleap_nn_amd import _lib as L

    lib = L.lib()
    a = np.zeros(4096, dtype=np.float64)
    cnt = np.zeros(64, dtype=np.int32)
    p, c = C.c_void_p(a.ctypes.data), C.c_void_p(cnt.ctypes.data)
    ok = lambda **kw: lib.ph_track_pose_scores(*[{**dict(cur=p, B=2, hist=p, L=2, n_hist=1, I=3, N=2, counts=c, method=0, std=0.025, out=p), **kw}[k]
                                                 for k in ("cur", "B", "hist", "L", "n_hist", "I", "N", "counts", "method", "std", "out")])
    assert ok() == L.PH_OK
    for bad in (dict(cur=None), dict(hist=None), dict(counts=None), dict(out=None), dict(B=0), dict(L=0), dict(L=33), dict(n_hist=3), dict(n_hist=-1), dict(I=0), dict(N=0),
                dict(method=4), dict(method=-1), dict(method=1, N=3)):
        assert ok(**bad) == L.PH_E_INVALID, bad
    cnt[1] = 4  # a count beyond I
    assert ok() == L.PH_E_INVALID
    assert b"counts" in lib.ph_last_error()


# ---- masks ----------------------------------------------------------------------------------------------------------

def mask_layer(full_res):
    from sleap_nn_amd.inference.layers.segmentation import SegmentationLayer
    from sleap_nn_amd.inference.preprocess_info import PreprocInfo

    layer = SegmentationLayer.__new__(SegmentationLayer)
    layer.full_res_masks, layer.min_mask_area, layer._axis_cache = bool(full_res), 0, {}
    g = PARAMS["mask_geometry"]
    info = PreprocInfo(original_size=tuple(g["original_size"]), processed_size=tuple(g["processed_size"]), eff_scale=torch.tensor([g["eff_scale"]]),
                       input_scale=g["input_scale"], output_stride=g["output_stride"])
    return layer, info


def mask_entries(label_map, full_res):
    layer, info = mask_layer(full_res)
    out, labels = [], []
    for k in range(int(label_map.max()) + 1):
        m = layer._package(label_map == k, 0.5 + 0.1 * k, info, 0)
        if m is not None:
            out.append(m), labels.append(k)
    return out, labels


@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("name", sorted(MASK_CASES))
def test_mask_case(name, batch):
    """The host mask path, frame by frame and through ``track_outputs`` in batches of 3 (no device here: host scoring): ids identical, scores EXACTLY equal."""
    from sleap_nn_amd.inference.outputs import Outputs
    from sleap_nn_amd.tracking import Tracker

    case = MASK_CASES[name]
    maps = Z["seq/masks/label_maps"]
    tr = Tracker.from_config(**case["kw"])
    for t0 in range(0, len(maps), batch):
        ents = [mask_entries(lm, case["full_res"])[0] for lm in maps[t0 : t0 + batch]]
        if batch == 1:
            ids, tsc = tr.track(ents[0], t0)
            check_frame(name, t0, tr, ids, tsc, 0.0, kind="mask")
            continue
        out = tr.track_outputs(Outputs(pred_masks=ents, frame_indices=torch.arange(t0, t0 + len(ents))))
        for b, fr in enumerate(out.pred_masks):
            e_ids, e_tsc, _ = expected(name, t0 + b)
            assert [m["track_id"] for m in fr] == e_ids.tolist()
            assert np.array_equal(np.array([m["tracking_score"] for m in fr]), e_tsc, equal_nan=True)
            assert "track_id" not in ents[b][0] if ents[b] else True  # the input entries stay as they were


@pytest.mark.parametrize("full_res", [False, True])
def test_axis_weights_give_the_image_grid_counts(full_res):
    """Counts with the bincount weights of the layer's per-axis index maps equal a brute-force IoU on explicitly decoded masks: non-uniform weights, zeros in the pad."""
    from sleap_nn_amd.tracking import scoring as S

    layer, info = mask_layer(full_res)
    maps = Z["seq/masks/label_maps"]
    h, w = maps.shape[1:]
    rows, cols = layer.axis_index_maps(info, 0, (h, w))
    rw, cw = S.axis_weights(rows, cols, h, w)
    oh, ow = PARAMS["mask_geometry"]["original_size"]
    assert rw.sum() == oh and cw.sum() == ow and len(set(rw[rw > 0].tolist())) > 1 and (rw[30:] == 0).all() and (cw[27:] == 0).all()
    weight = rw[:, None].astype(np.int64) * cw[None, :]
    for ta, tb in ((0, 1), (5, 6), (10, 13)):
        ea, la = mask_entries(maps[ta], full_res)
        eb, lb = mask_entries(maps[tb], full_res)
        for a, ka in zip(ea, la):
            da = S.decode_to_image(a)
            assert da.shape == (oh, ow)
            assert int(weight[maps[ta] == ka].sum()) == int(da.sum()) == S.mask_feature(a).area
            for b, kb in zip(eb, lb):
                db = S.decode_to_image(b)
                inter = int(weight[(maps[ta] == ka) & (maps[tb] == kb)].sum())
                assert inter == int((da & db).sum())
                union = int(da.sum()) + int(db.sum()) - inter
                iou = S.mask_iou_table(np.array([[inter]]), np.array([int(da.sum())]), np.array([int(db.sum())]))[0, 0]
                assert iou == S.mask_iou(a, b) == (inter / union if union else 1.0)
    assert S.mask_iou(np.zeros((4, 4), bool), np.zeros((4, 4), bool)) == 1.0


# ---- configuration --------------------------------------------------------------------------------------------------

def test_refusals_name_the_knob():
    from sleap_nn_amd.tracking import Tracker, TrackerConfig, resolve_config

    for kw, word in ((dict(use_flow=True), "use_flow"), (dict(use_kalman=True, tracking_target_instance_count=2), "use_kalman"), (dict(features="image"), "features='image'")):
        with pytest.raises(NotImplementedError, match=re.escape(word)):
            Tracker.from_config(**kw)
    with pytest.raises(ValueError, match="mutually exclusive"):
        Tracker.from_config(use_flow=True, use_kalman=True)
    with pytest.raises(ValueError, match="not a valid method"):
        Tracker.from_config(candidates_method="sliding")
    for kw, word in ((dict(tracking_clean_instance_count=2), "tracking_clean_instance_count"),
                     (dict(post_connect_single_breaks=True, tracking_target_instance_count=2), "post_connect_single_breaks")):
        with pytest.raises(NotImplementedError, match=word):
            resolve_config(TrackerConfig(**kw), 6, False)
    with pytest.raises(ValueError, match="tracking_target_instance_count"):
        resolve_config(TrackerConfig(tracking_pre_cull_to_target=1), 6, False)
    tr = Tracker.from_config(scoring_method="nope")
    with pytest.raises(ValueError, match="scoring_method"):
        tr.track(np.zeros((1, 2, 2)), 0)


def test_from_config_switch_and_defaults():
    from sleap_nn_amd.tracking import FixedWindowCandidates, LocalQueueCandidates, Tracker

    t = Tracker.from_config()
    assert isinstance(t.candidate, FixedWindowCandidates) and not t.is_local_queue and t.candidate.window_size == 5 and t.oks_stddev == 0.025
    assert (t.features, t.scoring_method, t.scoring_reduction, t.track_matching_method, t.min_match_points) == ("keypoints", "oks", "mean", "hungarian", 0)
    t = Tracker.from_config(max_tracks=3)  # the cap is only honoured by local_queues
    assert isinstance(t.candidate, LocalQueueCandidates) and t.is_local_queue and t.candidate.max_tracks == 3
    assert Tracker.from_config(oks_stddev=0.1).oks_stddev == 0.1
    # beyond max_tracks: -1 / NaN
    ids, tsc = Tracker.from_config(max_tracks=2).track(np.arange(36, dtype=np.float64).reshape(3, 6, 2) * np.array([1.0, 7.0, 19.0])[:, None, None], 0)
    assert ids.tolist() == [0, 1, -1] and np.isnan(tsc[2]) and tsc[:2].tolist() == [1.0, 1.0]


def test_apply_tracking_defaults():
    from sleap_nn_amd.inference.outputs import Outputs
    from sleap_nn_amd.tracking import TrackerConfig, apply_tracking, resolve_config

    auto = TrackerConfig(scoring_method_explicit=False, features_explicit=False, candidates_method_explicit=False)
    kw = resolve_config(auto, 1, False)  # a 1-node skeleton
    assert (kw["scoring_method"], kw["features"], kw["window_size"], kw["candidates_method"]) == ("euclidean_dist", "centroids", 5, "fixed_window")
    kw = resolve_config(TrackerConfig(), 1, False)  # explicit choices stay
    assert (kw["scoring_method"], kw["features"]) == ("oks", "keypoints")
    kw = resolve_config(auto, 6, False)
    assert (kw["scoring_method"], kw["features"]) == ("oks", "keypoints")
    kw = resolve_config(TrackerConfig(scoring_method_explicit=False, features_explicit=False, candidates_method_explicit=False, tracking_target_instance_count=4), None, True)
    assert (kw["scoring_method"], kw["features"], kw["window_size"], kw["candidates_method"], kw["max_tracks"]) == ("mask_iou", "masks", 25, "local_queues", 4)
    assert resolve_config(TrackerConfig(scoring_method_explicit=False, features_explicit=False, window_size=7), None, True)["window_size"] == 7
    with pytest.raises(ValueError, match="features='masks'"):
        resolve_config(TrackerConfig(), None, True)
    for kw in (dict(use_flow=True), dict(use_kalman=True)):
        with pytest.raises(ValueError, match="motion models"):
            resolve_config(TrackerConfig(scoring_method_explicit=False, features_explicit=False, **kw), None, True)
    with pytest.raises(ValueError, match="cull/clean/connect"):
        resolve_config(TrackerConfig(scoring_method_explicit=False, features_explicit=False, tracking_clean_instance_count=2), None, True)
    # batches handed over out of order are tracked in frame order and come back in the order given
    frames = pose_frames("plain")
    a, b = pose_outputs(frames, 0, 3), pose_outputs(frames, 3, 3)
    out = apply_tracking([b, a], TrackerConfig())
    for o, t0 in ((out[1], 0), (out[0], 3)):
        for k in range(3):
            n = len(frames[t0 + k][0])
            assert np.array_equal(o.instance_track_ids[k, :n].numpy(), Z[f"default/ids/{t0 + k}"])
    assert out[0].track_objects is out[1].track_objects
    # mask-only outputs resolve to the mask tracker
    ents = [mask_entries(lm, False)[0] for lm in Z["seq/masks/label_maps"][:3]]
    out = apply_tracking([Outputs(pred_masks=ents, frame_indices=torch.arange(3))], auto)
    assert [m["track_id"] for m in out[0].pred_masks[0]] == Z["mask_local_queues/ids/0"].tolist()


def test_outputs_attach_tracks(monkeypatch):
    """``to_instances`` / ``to_labels`` attach ``track_<id>`` tracks and tracking scores when ``instance_track_ids`` is set (a sleap-io stand-in: it is not installed here)."""
    import sys
    import types

    sio = types.ModuleType("sleap_io")

    class Track:
        def __init__(self, name=""):
            self.name = name

    class PredictedInstance:
        @classmethod
        def from_numpy(cls, **kw):
            o = cls()
            o.__dict__.update(kw)
            o.__dict__.setdefault("track", None)
            return o

    class LabeledFrame:
        def __init__(self, **kw):
            self.__dict__.update(kw)

    class Labels(LabeledFrame):
        pass

    sio.Track, sio.PredictedInstance, sio.LabeledFrame, sio.Labels = Track, PredictedInstance, LabeledFrame, Labels
    monkeypatch.setitem(sys.modules, "sleap_io", sio)
    from sleap_nn_amd.tracking import TrackerConfig, apply_tracking

    frames = pose_frames("plain")
    outs = apply_tracking([pose_outputs(frames, 0, 3), pose_outputs(frames, 3, 3)], TrackerConfig())
    skel = types.SimpleNamespace(nodes=list(range(6)))
    seen = {}
    for o, t0 in zip(outs, (0, 3)):
        labels = o.to_labels(skel)
        for b, lf in enumerate(labels.labeled_frames):
            e_ids, e_tsc, _ = expected("default", t0 + b)
            assert [int(i.track.name.split("_")[1]) for i in lf.instances] == e_ids.tolist()
            assert np.allclose([i.tracking_score for i in lf.instances], e_tsc, atol=TOL)
            for i in lf.instances:
                assert seen.setdefault(i.track.name, i.track) is i.track  # one Track object per id across the batches
        assert {t.name for t in labels.tracks} == {i.track.name for lf in labels.labeled_frames for i in lf.instances}
    # without a tracker nothing is attached
    lf = pose_outputs(frames, 0, 3).to_labels(skel).labeled_frames[0]
    assert all(i.track is None and "tracking_score" not in i.__dict__ for i in lf.instances)


def test_header_and_build_list_the_tracking_sources():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "posehip.h")).read()
    assert "ph_track_pose_scores" in header and "ph_track_mask_pairs" in header and "at or beyond P is treated as" in header
    assert int(re.search(r"^#define\s+PH_VERSION\s+(\d+)", header, re.M).group(1)) >= 117
    from sleap_nn_amd import build

    assert "track_host.cpp" in build.SOURCES and "track_kernels.hip" in build.SOURCES
