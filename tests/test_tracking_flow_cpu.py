"""The flow-shift tracker on the host (sleap_nn_amd/tracking/flow.py ``pyr_lk``, ``Tracker.from_config(use_flow=True, allow_flow=True)``).

``tests/golden/tracking_flow.npz`` comes from the reference's own ``FlowShiftTracker`` run over ``pyr_lk`` as its ``cv2.calcOpticalFlowPyrLK``
(tools/gen_tracking_flow_golden.py): it pins the tracker's logic, not OpenCV's numbers.  Frames and poses are regenerated from seeds by ``tests/_flow.py``.
"""
import json
import os
import re

import numpy as np
import pytest
import torch

from tests import _flow as TF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Z = np.load(os.path.join(ROOT, "tests", "golden", "tracking_flow.npz"))
PARAMS = json.loads(str(Z["params"]))
CASES = PARAMS["cases"]


def case_kw(name):
    return dict(PARAMS["of"], use_flow=True, allow_flow=True, **CASES[name]["kw"])


def case_sequence(name):
    return TF.flow_sequence(PARAMS["seeds"][name], CASES[name]["seq"])


def expected(name, t):
    key = f"{name}/scores/{t}"
    return Z[f"{name}/ids/{t}"], Z[f"{name}/tracking_scores/{t}"], Z[key] if key in Z else None


def flow_outputs(seq, t0, n):
    from sleap_nn_amd.inference.outputs import Outputs

    chunk = seq[t0 : t0 + n]
    I = max(len(p) for p, _s in chunk) + 1  # one NaN-padded slot more than the fullest frame
    kp = torch.full((len(chunk), I, chunk[0][0].shape[1], 2), float("nan"), dtype=torch.float64)
    sc = torch.full((len(chunk), I), float("nan"), dtype=torch.float64)
    valid = torch.zeros((len(chunk), I), dtype=torch.bool)
    for b, (p, s) in enumerate(chunk):
        kp[b, : len(p)], sc[b, : len(p)], valid[b, : len(p)] = torch.from_numpy(p), torch.from_numpy(s), True
    return Outputs(pred_keypoints=kp, instance_scores=sc, instance_valid=valid, frame_indices=torch.arange(t0, t0 + len(chunk)))


# ---- the pyramid ----------------------------------------------------------------------------------------------------

def test_pyramid_sizes_and_early_stop():
    from sleap_nn_amd.tracking.flow import build_pyramid, pyramid_shapes

    assert pyramid_shapes(64, 80, 9, 3) == [(64, 80), (32, 40), (16, 20)]  # (8, 10) does not exceed win = 9: three levels, not four
    assert pyramid_shapes(97, 131, 9, 3) == [(97, 131), (49, 66), (25, 33), (13, 17)]  # odd sides halve upward
    assert pyramid_shapes(96, 128, 21, 3) == [(96, 128), (48, 64), (24, 32)]
    assert pyramid_shapes(96, 128, 21, 1) == [(96, 128), (48, 64)] and pyramid_shapes(96, 128, 21, 0) == [(96, 128)]
    assert pyramid_shapes(40, 400, 21, 7) == [(40, 400)]  # one side at or below win ends it
    img = TF.texture(3, 97, 131)
    assert [l.shape for l in build_pyramid(img, 9, 3)] == pyramid_shapes(97, 131, 9, 3) and all(l.dtype == np.uint8 for l in build_pyramid(img, 9, 3))


def test_reflect_borders_and_downsampling():
    from sleap_nn_amd.tracking.flow import pyr_down, reflect101, scharr

    assert reflect101(np.arange(-3, 8), 5).tolist() == [3, 2, 1, 0, 1, 2, 3, 4, 3, 2, 1]
    assert reflect101(np.array([-9, 13]), 5).tolist() == [1, 3] and reflect101(np.array([-2, 5]), 1).tolist() == [0, 0]
    img = TF.texture(4, 13, 18)
    pad = np.pad(img.astype(np.int64), 2, mode="reflect")  # (NumPy's "reflect" is reflect-101)
    k = np.array([1, 4, 6, 4, 1])
    want = np.zeros((7, 9), dtype=np.int64)
    for y in range(7):
        for x in range(9):
            want[y, x] = ((pad[2 * y : 2 * y + 5, 2 * x : 2 * x + 5] * np.outer(k, k)).sum() + 128) >> 8
    assert np.array_equal(pyr_down(img), want.astype(np.uint8))
    assert np.array_equal(pyr_down(np.full((10, 12), 77, np.uint8)), np.full((5, 6), 77, np.uint8))  # the taps sum to 256
    gx, gy = scharr(img)
    p1 = np.pad(img.astype(np.int64), 1, mode="reflect")
    y, x = 0, 17  # a corner: every tap outside the image is a reflected pixel
    assert gx[y, x] == 3 * p1[y, x + 2] + 10 * p1[y + 1, x + 2] + 3 * p1[y + 2, x + 2] - 3 * p1[y, x] - 10 * p1[y + 1, x] - 3 * p1[y + 2, x] == 0
    assert gy[6, 5] == 3 * p1[8, 5] + 10 * p1[8, 6] + 3 * p1[8, 7] - 3 * p1[6, 5] - 10 * p1[6, 6] - 3 * p1[6, 7]
    ramp = np.tile(np.arange(20, dtype=np.uint8) * 3, (9, 1))
    gx, gy = scharr(ramp)
    assert (gx[:, 1:-1] == 16 * 6).all() and (gx[:, [0, -1]] == 0).all() and (gy == 0).all()


# ---- pyr_lk ---------------------------------------------------------------------------------------------------------

def test_pyr_lk_recovers_known_translations():
    """The bar is twice the largest error the stand-in itself shows on these inputs, as the generator measured and recorded it (0.0195 px -> 0.039 px)."""
    from sleap_nn_amd.tracking.flow import pyr_lk

    bar = 2 * PARAMS["stand_in_max_error_px"]
    assert 0.01 < bar < 0.15
    worst = 0.0
    for seed, sh in enumerate(PARAMS["translations"], start=1):
        a, b = TF.texture(seed, 96, 128), TF.texture(seed, 96, 128, sh)
        pts = TF.interior_points(seed + 50, 40, 96, 128, 28)
        got, status = pyr_lk(a, b, pts)
        assert status.dtype == np.uint8 and status.all() and got.dtype == np.float32
        worst = max(worst, float(np.linalg.norm(got - pts - np.float32(sh), axis=1).max()))
    print(f"largest error against known translations: {worst:.4f} px (bar {bar:.4f})")
    assert worst <= bar
    a, b = TF.texture(2, 96, 128), TF.texture(2, 96, 128, (2.5, -1.5))
    pts = TF.interior_points(9, 30, 96, 128, 20)
    for win in (9, 5):  # smaller windows, more levels: 25 quantised pixels no longer average the rounding away, so only "the right pixel" is asked (half a pixel)
        got, status = pyr_lk(a, b, pts, win=win)
        assert status.all() and np.linalg.norm(got - pts - np.float32((2.5, -1.5)), axis=1).max() < 0.5


def test_pyr_lk_lost_points_are_deterministic():
    from sleap_nn_amd.tracking.flow import pyr_lk

    a = TF.texture(1, 96, 128, flat=(20, 70, 30, 90))
    b = TF.texture(1, 96, 128, (1.0, 0.5), flat=(20, 70, 30, 90))
    pts = np.array([[60, 45], [-30, 40], [158, 20], [64, -30], [64, 126], [np.nan, 3], [7, np.nan], [110, 80]], dtype=np.float32)
    got, status = pyr_lk(a, b, pts, max_level=0)
    # a window over an exactly flat region has A = 0; 30 px outside the frame; NaN; the last point is ordinary
    assert status.tolist() == [0, 0, 0, 0, 0, 0, 0, 1]
    assert np.isnan(got[:7]).all() and np.linalg.norm(got[7] - pts[7] - np.float32((1.0, 0.5))) < 0.1
    again, status2 = pyr_lk(a, b, pts, max_level=0)
    assert np.array_equal(got, again, equal_nan=True) and np.array_equal(status, status2)
    got3, status3 = pyr_lk(a, b, pts[[1, 2, 5]])  # with the pyramid: still lost (the level-0 bounds test)
    assert status3.tolist() == [0, 0, 0] and np.isnan(got3).all()
    empty, st = pyr_lk(a, b, np.zeros((0, 2), np.float32))
    assert empty.shape == (0, 2) and st.shape == (0,)


def test_shifted_pair_scores_match_the_pair_functions():
    from sleap_nn_amd.tracking import Tracker
    from sleap_nn_amd.tracking import scoring as S

    g = np.random.default_rng(5)
    B, L, I, N = 2, 3, 4, 5
    cur, hist = g.uniform(0, 50, (B, I, N, 2)), g.uniform(0, 50, (B, L, I, N, 2))
    cur[0, 1, 2], hist[1, 0, 2, 3] = np.nan, np.nan
    cc, ch = np.array([4, 3], np.int32), np.array([[4, 0, 2], [1, 4, 3]], np.int32)
    for method in ("oks", "euclidean_dist", "cosine_sim"):
        tr = Tracker.from_config(scoring_method=method)
        flat = method != "oks"
        got = S.pose_pair_scores_shifted(cur, hist, cc, ch, method, 0.025)
        for b in range(B):
            for l in range(L):
                for i in range(I):
                    for j in range(I):
                        if i < cc[b] and j < ch[b, l]:
                            a, p = (cur[b, i].ravel(), hist[b, l, j].ravel()) if flat else (cur[b, i], hist[b, l, j])
                            np.testing.assert_allclose(got[b, l, i, j], tr.pair_score(a, p), rtol=1e-12, equal_nan=True)
                        else:
                            assert np.isnan(got[b, l, i, j])


# ---- the tracker ----------------------------------------------------------------------------------------------------

def test_flow_tracker_constructs_only_with_the_opt_in():
    from sleap_nn_amd.tracking import Tracker, TrackerConfig, resolve_config

    tr = Tracker.from_config(use_flow=True, allow_flow=True)
    assert tr.use_flow and tr.of_window_size == 21 and tr.of_max_levels == 3 and not tr.is_local_queue
    assert Tracker.from_config(use_flow=True, allow_flow=True, max_tracks=3).is_local_queue
    assert not Tracker.from_config(allow_flow=True).use_flow
    with pytest.raises(NotImplementedError, match="allow_flow"):
        Tracker.from_config(use_flow=True)
    assert TrackerConfig().allow_flow is False and list(TrackerConfig.__dataclass_fields__)[-1] == "allow_flow"
    kw = resolve_config(TrackerConfig(use_flow=True, allow_flow=True, of_window_size=15), 4, False)
    assert kw["allow_flow"] is True and Tracker.from_config(**kw).of_window_size == 15


def test_refusals_that_remain():
    from sleap_nn_amd.tracking import Tracker, TrackerConfig, apply_tracking, resolve_config

    with pytest.raises(NotImplementedError, match="use_flow"):
        Tracker.from_config(use_flow=True)
    with pytest.raises(NotImplementedError, match="of_img_scale"):
        Tracker.from_config(use_flow=True, allow_flow=True, of_img_scale=0.5)
    with pytest.raises(NotImplementedError, match=re.escape("features='image'")):
        Tracker.from_config(use_flow=True, allow_flow=True, features="image")
    with pytest.raises(NotImplementedError, match="use_kalman"):
        Tracker.from_config(use_kalman=True, allow_flow=True)
    with pytest.raises(ValueError, match="mutually exclusive"):
        Tracker.from_config(use_flow=True, use_kalman=True, allow_flow=True)
    with pytest.raises(ValueError, match="of_window_size"):
        Tracker.from_config(use_flow=True, allow_flow=True, of_window_size=43)
    with pytest.raises(ValueError, match="of_max_levels"):
        Tracker.from_config(use_flow=True, allow_flow=True, of_max_levels=8)
    with pytest.raises(ValueError, match="motion models"):
        resolve_config(TrackerConfig(use_flow=True, allow_flow=True, scoring_method_explicit=False, features_explicit=False), None, True)
    tr = Tracker.from_config(use_flow=True, allow_flow=True)
    tr.flow_device = False
    pts = np.array([[[30.0, 30.0], [40.0, 35.0]]])
    with pytest.raises(ValueError, match="image"):
        tr.track(pts, 0)
    with pytest.raises(NotImplementedError, match="more than one channel"):
        tr.track(pts, 0, image=np.zeros((64, 64, 3), np.uint8))
    with pytest.raises(ValueError, match="frames"):
        apply_tracking([flow_outputs([(pts[0][None], np.ones(1))], 0, 1)], TrackerConfig(use_flow=True, allow_flow=True))
    with pytest.raises(NotImplementedError, match="allow_flow"):
        apply_tracking([flow_outputs([(pts[0][None], np.ones(1))], 0, 1)], TrackerConfig(use_flow=True), frames=np.zeros((1, 64, 64), np.uint8))


def test_frame_shapes_and_float_frames():
    from sleap_nn_amd.tracking import Tracker

    frames, seq = case_sequence("fixed_hungarian")
    res = []
    for wrap in (lambda f: f, lambda f: f[:, :, None], lambda f: f[None], lambda f: f.astype(np.float32) + 0.75, lambda f: torch.from_numpy(f)):
        tr = Tracker.from_config(**case_kw("fixed_hungarian"))
        tr.flow_device = False
        res.append([tr.track(p, t, s, image=wrap(frames[t])) for t, (p, s) in enumerate(seq[:4])])
    for other in res[1:]:  # a float frame is truncated to uint8: the same pixels
        for (i0, s0), (i1, s1) in zip(res[0], other):
            assert np.array_equal(i0, i1) and np.array_equal(s0, s1, equal_nan=True)


@pytest.mark.parametrize("name", sorted(CASES))
def test_flow_case_frame_by_frame(name):
    from sleap_nn_amd.tracking import Tracker

    frames, seq = case_sequence(name)
    tr = Tracker.from_config(**case_kw(name))
    tr.flow_device = False
    for t, (p, s) in enumerate(seq):
        ids, tsc = tr.track(p, t, s, image=frames[t])
        e_ids, e_tsc, e_sc = expected(name, t)
        assert np.array_equal(ids, e_ids), (name, t)
        np.testing.assert_allclose(tsc, e_tsc, rtol=1e-9, atol=0, equal_nan=True)
        if e_sc is not None:
            np.testing.assert_allclose(tr.last_scores, e_sc, rtol=1e-9, atol=0, equal_nan=True)
    assert tr.flow_cpu_calls > 0 and tr.flow_launches == 0


@pytest.mark.parametrize("batch", [1, 4])
@pytest.mark.parametrize("name", sorted(CASES))
def test_flow_case_in_batches(name, batch):
    from sleap_nn_amd.tracking import Tracker

    frames, seq = case_sequence(name)
    tr = Tracker.from_config(**case_kw(name))
    tr.flow_device = False
    for t0 in range(0, len(seq), batch):
        out = tr.track_outputs(flow_outputs(seq, t0, batch), images=frames[t0 : t0 + batch])
        for b in range(out.batch_size):
            e_ids, e_tsc, _ = expected(name, t0 + b)
            n = len(e_ids)
            assert np.array_equal(out.instance_track_ids[b, :n].numpy(), e_ids), (name, t0 + b)
            assert (out.instance_track_ids[b, n:] == -1).all()
            np.testing.assert_allclose(out.instance_tracking_scores[b, :n].numpy(), e_tsc, rtol=1e-9, atol=0, equal_nan=True)
    if not tr.is_local_queue:
        assert tr.table_hits > 0  # the fixed window reads the batch's table
        if batch == 4 and tr.candidate.window_size >= 3:
            assert tr.pair_calls == 0


def test_golden_tells_flow_from_plain_tracking():
    from sleap_nn_amd.tracking import Tracker

    frames, seq = case_sequence("close_euclid")
    kw = {k: v for k, v in case_kw("close_euclid").items() if k not in ("use_flow", "allow_flow", "of_window_size", "of_max_levels")}
    tr = Tracker.from_config(**kw)
    plain = [tr.track(p, t, s)[0] for t, (p, s) in enumerate(seq)]
    assert any(not np.array_equal(i, expected("close_euclid", t)[0]) for t, i in enumerate(plain))
    assert PARAMS["lost_nodes"]["lost_points"] > 0 and "stand-in" in PARAMS["note"]  # (nodes with a position in the source that the flow lost)


def test_apply_tracking_hands_the_frames_on():
    from sleap_nn_amd.tracking import TrackerConfig, apply_tracking

    frames, seq = case_sequence("fixed_hungarian")
    cfg = TrackerConfig(use_flow=True, allow_flow=True, **PARAMS["of"])
    outs = [flow_outputs(seq, t0, 4) for t0 in range(0, len(seq), 4)]
    import sleap_nn_amd.tracking.tracker as T

    made = []
    orig = T.Tracker.__init__

    def init(self, *a, **k):
        orig(self, *a, **k)
        self.flow_device = False
        made.append(self)

    T.Tracker.__init__ = init
    try:
        tracked = apply_tracking(outs[::-1], cfg, frames=torch.from_numpy(frames)[:, None])[::-1]  # (N, 1, H, W), batches handed over out of order
    finally:
        T.Tracker.__init__ = orig
    for k, o in enumerate(tracked):
        for b in range(o.batch_size):
            e_ids = expected("fixed_hungarian", 4 * k + b)[0]
            assert np.array_equal(o.instance_track_ids[b, : len(e_ids)].numpy(), e_ids)
    assert len(made) == 1 and made[0].use_flow


def test_header_signatures_and_build_list_the_flow_sources():
    header = open(os.path.join(ROOT, "include", "posehip.h")).read()
    from sleap_nn_amd import _lib, build

    for name in ("ph_flow_pyramid", "ph_flow_track", "ph_flow_levels", "ph_flow_job_size", "ph_track_pose_scores_shifted"):
        assert re.search(rf"\b{name}\(", header) and name in _lib.SIGNATURES and hasattr(_lib.lib(), name)
    assert int(re.search(r"^#define\s+PH_VERSION\s+(\d+)", header, re.M).group(1)) >= 122
    assert "flow_kernels.hip" in build.SOURCES
    from sleap_nn_amd.tracking.flow import MAX_LEVELS, JobDesc
    import ctypes as C

    assert _lib.lib().ph_flow_job_size() == C.sizeof(JobDesc) == 16 * MAX_LEVELS + 8
    sizes = (C.c_int32 * 16)()
    assert _lib.lib().ph_flow_levels(64, 80, 9, 3, C.cast(sizes, C.c_void_p)) == 3 and list(sizes[:6]) == [64, 80, 32, 40, 16, 20]
    for bad in ((64, 80, 2, 3), (64, 80, 43, 3), (64, 80, 9, 8), (64, 80, 9, -1), (1, 80, 9, 3)):
        assert _lib.lib().ph_flow_levels(*bad, None) == _lib.PH_E_INVALID
