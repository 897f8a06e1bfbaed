"""The flow-shift tracker on the GPU: ``ph_flow_pyramid`` / ``ph_flow_track`` (csrc/flow_kernels.hip) against ``sleap_nn_amd.tracking.flow.pyr_lk``, the
definition; the device tracker against the golden of ``tests/test_tracking_flow_cpu.py`` and against the host path; ``Predictor`` end to end.

Frames are the seeded textures of ``tests/_flow.py`` at 96 x 128, 97 x 131 (odd halving) and 64 x 80 (the pyramid stops early at ``win = 9``): small enough for
milliseconds, large enough for every level, more than one workgroup per job and a window (``win = 21``: 441 pixels) of several rounds per lane.
"""
import json
import os

import numpy as np
import pytest
import torch

from tests import _flow as TF

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Z = np.load(os.path.join(ROOT, "tests", "golden", "tracking_flow.npz"))
PARAMS = json.loads(str(Z["params"]))
H, W = 96, 128
FLAT = (20, 76, 30, 98)  # (y0, y1, x0, x1) of the reference frames' region without gradient
SHIFTS = [(0.0, 0.0), (2.6, -1.3), (5.1, 1.8)]


@pytest.mark.parametrize("h,w,win,max_level", [(96, 128, 21, 3), (97, 131, 9, 3), (64, 80, 9, 3), (97, 131, 5, 7), (96, 128, 21, 0)])
def test_pyramid_is_bit_identical(h, w, win, max_level):
    from sleap_nn_amd.tracking.flow import build_pyramid, pyramid_device, pyramid_shapes

    frames = np.stack([TF.texture(20 + b, h, w) for b in range(3)])
    dev = pyramid_device(torch.from_numpy(frames).to(DEV), win, max_level)
    assert len(dev) == 3
    for b in range(3):
        ref = build_pyramid(frames[b], win, max_level)
        assert [tuple(l.shape) for l in dev[b]] == pyramid_shapes(h, w, win, max_level) == [l.shape for l in ref]
        for l, (got, want) in enumerate(zip(dev[b], ref)):
            assert got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), want), (b, l)


def flow_frames():
    return np.stack([TF.texture(31, H, W, s, flat=FLAT) for s in SHIFTS])


def candidate_points(seed, win):
    """65 points of every kind; ``robust_points`` keeps those whose status cannot hang on a last bit."""
    g = np.random.default_rng(seed)
    half = (win - 1) / 2
    interior = TF.interior_points(seed, 24, H, W, half + 8)
    edge = g.uniform(0, 3, 16)
    along_x, along_y = g.uniform(5, W - 6, 16), g.uniform(5, H - 6, 16)
    border = np.stack([np.where(np.arange(16) % 4 == 0, edge, np.where(np.arange(16) % 4 == 1, W - 1 - edge, along_x)),
                       np.where(np.arange(16) % 4 == 2, edge, np.where(np.arange(16) % 4 == 3, H - 1 - edge, along_y))], axis=1)
    outside = np.array([[-30, 40], [W + 29, 50], [60, -30], [70, H + 29], [-30, -30], [-60, 40], [W + 59, 50], [60, -60], [70, H + 59]], dtype=np.float64)  # (at 60 px the coarse levels' tests are clear too)
    nan = np.array([[np.nan, 20], [30, np.nan], [np.nan, np.nan]])
    flat = np.stack([g.uniform(FLAT[2] + half + 4, FLAT[3] - half - 5, 8), g.uniform(FLAT[0] + half + 4, FLAT[1] - half - 5, 8)], axis=1)
    kinds = ["interior"] * 24 + ["border"] * 16 + ["outside"] * 9 + ["nan"] * 3 + ["flat"] * 8
    return np.concatenate([interior, border, outside, nan, flat]).astype(np.float32), np.array(kinds)


def robust_points(ref, cur, pts, kinds, win, max_level):
    """Status must be EQUAL on every point, so the points are those whose stand-in ``minEig`` is exactly 0 or at least 10 times the threshold at every level
    that computed one, and whose every bounds test stays 2 px clear of flipping."""
    from sleap_nn_amd.tracking.flow import pyr_lk

    info = {}
    shifted, status = pyr_lk(ref, cur, pts, win, max_level, info=info)
    eig = info["min_eig"]
    keep = (np.isnan(eig) | (eig == 0) | (eig >= 1e-3)).all(axis=1) & (info["margin"] >= 2.0)
    return keep, shifted, status


@pytest.mark.parametrize("win", [21, 9, 5])
def test_flow_track_against_pyr_lk(win):
    """B = 3 frames, 2 lags (both directions: 6 jobs), about 40 points per job: interior, within 3 px of each border, 30 px outside the frame, NaN, and on a flat
    region.  Status EQUAL on every point; shifted points within 0.02 px, twice the stop radius: two correct evaluations can differ by one termination decision,
    the last step of at most 0.01 px plus the half-step back.  Measured maximum on an MI355X: 0.000000 px at each of win 21 / 9 / 5 (321 / 254 / 207 points:
    bit-equal to ``pyr_lk``); DESIGN.md 4.2g."""
    from sleap_nn_amd.tracking.flow import pyramid_device, track_device

    max_level = 3
    frames = flow_frames()
    pyr = pyramid_device(torch.from_numpy(frames).to(DEV), win, max_level)
    pairs = [(1, 0), (2, 1), (2, 0), (0, 1), (1, 2), (0, 2)]  # (current, reference)
    jobs, want = [], []
    seen = {k: 0 for k in ("interior", "border", "outside", "nan", "flat")}
    for j, (c, r) in enumerate(pairs):
        pts, kinds = candidate_points(100 * win + j, win)
        keep, shifted, status = robust_points(frames[r], frames[c], pts, kinds, win, max_level)
        for k in kinds[keep]:
            seen[k] += 1
        assert keep.sum() >= 25
        jobs.append((pyr[r], pyr[c], pts[keep]))
        want.append((shifted[keep], status[keep], kinds[keep]))
    assert min(seen.values()) >= 6, seen  # every kind is present
    got = track_device(jobs, win, max_level)
    worst = 0.0
    for (g_sh, g_st), (w_sh, w_st, kinds) in zip(got, want):
        assert g_st.dtype == np.uint8 and g_sh.dtype == np.float32 and np.array_equal(g_st, w_st), (kinds[g_st != w_st], win)
        found = w_st.astype(bool)
        assert np.isnan(g_sh[~found]).all() and not found[np.isin(kinds, ("outside", "nan", "flat"))].any() and found[kinds == "interior"].sum() >= 8
        if found.any():
            worst = max(worst, float(np.linalg.norm(g_sh[found] - w_sh[found], axis=1).max()))
    print(f"win {win}: largest distance between ph_flow_track and pyr_lk {worst:.6f} px over {sum(len(w[1]) for w in want)} points")
    assert worst <= 0.02


def test_one_launch_equals_the_jobs_one_by_one():
    from sleap_nn_amd.tracking.flow import pyramid_device, track_device

    frames = flow_frames()
    pyr = pyramid_device(torch.from_numpy(frames).to(DEV), 21, 3)
    jobs = [(pyr[r], pyr[c], candidate_points(7 + c, 21)[0][: 40 - 7 * c]) for c, r in [(1, 0), (2, 1), (2, 0)]]  # (jobs of 40, 26 and 26 points)
    together = track_device(jobs, 21, 3)
    for job, (sh, st) in zip(jobs, together):
        one_sh, one_st = track_device([job], 21, 3)[0]
        assert np.array_equal(sh.view(np.uint32), one_sh.view(np.uint32)) and np.array_equal(st, one_st)
    again = track_device(jobs, 21, 3)
    assert all(np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)) for a, b in zip(together, again))


def test_argument_checks():
    from sleap_nn_amd import _lib as L
    from sleap_nn_amd.tracking.flow import pyramid_device, track_device

    frames = torch.from_numpy(flow_frames()).to(DEV)
    pts = np.array([[40.0, 40.0]], np.float32)
    for win, lv in ((2, 3), (43, 3), (21, 8), (21, -1)):
        with pytest.raises(L.PosehipError):
            pyramid_device(frames, win, lv)
    pyr = pyramid_device(frames, 21, 3)
    for win, lv in ((2, 3), (43, 3), (21, 8)):
        with pytest.raises(L.PosehipError):
            track_device([(pyr[0], pyr[1], pts)], win, lv)
    with pytest.raises(L.PosehipError):
        track_device([(pyr[0], pyr[1], pts)], 21, 3, max_iter=0)
    assert track_device([(pyr[0], pyr[1], np.zeros((0, 2), np.float32))], 21, 3)[0][0].shape == (0, 2)
    torch.cuda.synchronize()


@pytest.mark.parametrize("name", sorted(PARAMS["cases"]))
def test_device_tracker_gives_the_golden_ids_and_the_host_path_ids(name):
    from sleap_nn_amd.tracking import Tracker
    from tests.test_tracking_flow_cpu import case_kw, case_sequence, expected, flow_outputs

    frames, seq = case_sequence(name)
    dev_frames = torch.from_numpy(frames).to(DEV)
    on_dev, on_host = Tracker.from_config(**case_kw(name)), Tracker.from_config(**case_kw(name))
    on_host.flow_device = False
    for t0 in range(0, len(seq), 4):
        outs = flow_outputs(seq, t0, 4)
        a = on_dev.track_outputs(outs, images=dev_frames[t0 : t0 + 4])
        b = on_host.track_outputs(outs, images=frames[t0 : t0 + 4])
        assert torch.equal(a.instance_track_ids, b.instance_track_ids), (name, t0)
        for k in range(a.batch_size):
            e_ids = expected(name, t0 + k)[0]
            assert np.array_equal(a.instance_track_ids[k, : len(e_ids)].numpy(), e_ids), (name, t0 + k)
        sa, sb = a.instance_tracking_scores.numpy(), b.instance_tracking_scores.numpy()
        assert np.array_equal(np.isnan(sa), np.isnan(sb))
    assert on_dev.flow_launches > 0 and on_dev.flow_cpu_calls == 0 and on_host.flow_launches == 0
    if not on_dev.is_local_queue:
        assert on_dev.flow_launches == 3  # ONE launch per batch for all (frame, lag, instance) flows
    # frame by frame with host frames: uploaded, one launch per frame
    single = Tracker.from_config(**case_kw(name))
    for t, (p, s) in enumerate(seq):
        ids, _tsc = single.track(p, t, s, image=frames[t])
        assert np.array_equal(ids, expected(name, t)[0]), (name, t)
    assert single.flow_launches > 0 and single.flow_cpu_calls == 0


def test_predictor_end_to_end_with_a_flow_config():
    from oracle import cpu_ref as O
    from sleap_nn_amd.architectures.model import Model
    from sleap_nn_amd.inference.backends import HipBackend
    from sleap_nn_amd.inference.layers import PostprocessConfig, SingleInstanceLayer
    from sleap_nn_amd.inference.predictor import Predictor
    from sleap_nn_amd.tracking import TrackerConfig

    bb = {"in_channels": 1, "kernel_size": 3, "filters": 8, "filters_rate": 2, "max_stride": 16, "stem_stride": None, "middle_block": True, "up_interpolate": True,
          "stacks": 1, "convs_per_block": 2, "output_stride": 2}
    heads = {"confmaps": {"part_names": ["a", "b", "c"], "sigma": 2.5, "output_stride": 2, "loss_weight": 1.0}}
    m = Model("unet", bb, heads, "single_instance")
    m.load_state_dict(O.init_state(bb, heads, "single_instance", seed=3, head_scale=1.0))
    layer = SingleInstanceLayer(HipBackend(m, DEV), 2, max_stride=16, postprocess_config=PostprocessConfig(peak_threshold=-1.0))
    frames = np.stack([TF.texture(8, 64, 96, (1.5 * t, 0.5 * t)) for t in range(5)])[:, None]  # (5, 1, 64, 96) uint8
    cfg = TrackerConfig(use_flow=True, allow_flow=True, of_window_size=15, scoring_method_explicit=False, features_explicit=False)
    outs = Predictor(layer, batch_size=2, tracker_config=cfg).predict(frames)
    assert len(outs) == 3
    ids = torch.cat([o.instance_track_ids for o in outs])
    assert ids.shape == (5, 1) and ids.dtype == torch.int64 and (ids == 0).all()  # one animal: one identity throughout
    assert all(o.instance_tracking_scores is not None for o in outs)
    with pytest.raises(NotImplementedError, match="allow_flow"):
        Predictor(layer, batch_size=2, tracker_config=TrackerConfig(use_flow=True, of_window_size=15, scoring_method_explicit=False, features_explicit=False)).predict(frames)
