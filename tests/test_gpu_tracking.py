"""Cross-frame tracking on the GPU: ``ph_track_mask_pairs`` (csrc/track_kernels.hip) against a NumPy brute force -- exact: the sums are integers --, its
run-to-run and stream-to-stream identity and its argument checks; the device-table mask tracker against the host-scoring tracker on label maps that
``SegmentationLayer.postprocess`` produced on the device; a run directory through ``Predictor`` with and without a tracker.

Shapes are the smallest that can break the kernel: 37 x 53 maps (no multiple of the 8-cell groups), more than one frame and lag, ``P`` of 1, 5 and 64, every label
width, non-uniform weights with zeros in the padding, a label equal to ``P`` (background by contract), an all-background frame, the history branch ``b < k`` with
``n_hist`` of 0, 2, 3 (the ring of two consecutive batches) and 4."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests import _golden as G

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
H, W, B, L = 37, 53, 3, 4
DT = {1: torch.int8, 2: torch.int16, 4: torch.int32}


def weights(g):
    rw = g.integers(1, 5, H).astype(np.int32)
    cw = g.integers(1, 4, W).astype(np.int32)
    rw[33:], cw[47:] = 0, 0  # the padding
    rw[5], cw[11] = 0, 0  # (a nearest resample may skip a cell row / column when it shrinks)
    return rw, cw


def random_maps(g, n, P):
    m = g.integers(-1, P + 1, (n, H, W))  # P itself is present: background by contract
    m[g.uniform(size=m.shape) < 0.4] = -1
    for f in range(n):  # blocks of one label: runs along a row
        y, x = int(g.integers(0, H - 8)), int(g.integers(0, W - 12))
        m[f, y : y + 8, x : x + 12] = int(g.integers(0, P))
    return m


def brute(cur, hist, n_hist, rw, cw, P):
    wt = rw[:, None].astype(np.int64) * cw[None, :]
    inter = np.zeros((len(cur), L, P, P), dtype=np.int64)
    area = np.zeros((len(cur), P), dtype=np.int64)
    for b in range(len(cur)):
        for a in range(P):
            area[b, a] = wt[cur[b] == a].sum()
        for k in range(1, L + 1):
            past = cur[b - k] if b >= k else (hist[L - (k - b)] if k - b <= n_hist else None)
            if past is None:
                continue
            for a in range(P):
                for c in range(P):
                    inter[b, k - 1, a, c] = wt[(cur[b] == a) & (past == c)].sum()
    return inter, area


def brute_fast(cur, hist, n_hist, rw, cw, P):
    """The same sums by one bincount per (b, k) (P = 64 has 4096 pairs)."""
    wt = (rw[:, None].astype(np.int64) * cw[None, :]).reshape(-1)
    inter = np.zeros((len(cur), L, P, P), dtype=np.int64)
    area = np.zeros((len(cur), P), dtype=np.int64)
    ok = lambda m: (m >= 0) & (m < P)
    for b in range(len(cur)):
        a = cur[b].reshape(-1)
        area[b] = np.bincount(a[ok(a)], weights=wt[ok(a)], minlength=P)
        for k in range(1, L + 1):
            past = cur[b - k] if b >= k else (hist[L - (k - b)] if k - b <= n_hist else None)
            if past is None:
                continue
            c = past.reshape(-1)
            sel = ok(a) & ok(c)
            inter[b, k - 1] = np.bincount(a[sel] * P + c[sel], weights=wt[sel], minlength=P * P).reshape(P, P)
    return inter, area


def run(cur, hist, n_hist, rw, cw, P, nbytes, stream=None):
    from sleap_nn_amd.tracking import scoring as S

    c, h = torch.from_numpy(cur).to(DT[nbytes]).to(DEV), torch.from_numpy(hist).to(DT[nbytes]).to(DEV)
    r, w_ = torch.from_numpy(rw).to(DEV), torch.from_numpy(cw).to(DEV)
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream(DEV)):
        rec, inter, area = S.mask_pair_counts(c, h, n_hist, r, w_, P, int(rw.sum()) * int(cw.sum()))
    torch.cuda.synchronize()
    return inter.cpu().numpy(), area.cpu().numpy()


@pytest.mark.parametrize("nbytes", [1, 2, 4])
@pytest.mark.parametrize("P", [1, 5, 64])
def test_mask_pairs_equal_brute_force(P, nbytes):
    g = np.random.default_rng(100 * P + nbytes)
    rw, cw = weights(g)
    first, second = random_maps(g, B, P), random_maps(g, B, P)
    second[1] = -1  # an all-background frame
    junk = random_maps(g, L, P)  # never read at n_hist = 0
    if P == 5:  # the two brute forces agree (the plain one is the definition)
        for n_hist in (0, 4):
            a, b_ = brute(first, junk, n_hist, rw, cw, P), brute_fast(first, junk, n_hist, rw, cw, P)
            assert np.array_equal(a[0], b_[0]) and np.array_equal(a[1], b_[1])
    inter, area = run(first, junk, 0, rw, cw, P, nbytes)
    e_inter, e_area = brute_fast(first, junk, 0, rw, cw, P)
    assert np.array_equal(inter, e_inter) and np.array_equal(area, e_area)
    assert not inter[0].any() and not inter[1, 1:].any() and e_area.any()  # lags beyond the history are zeros
    # the second batch against the ring the first left: newest last, 3 of the 4 slots valid
    ring = np.concatenate([junk, first])[-L:]
    inter, area = run(second, ring, B, rw, cw, P, nbytes)
    e_inter, e_area = brute_fast(second, ring, B, rw, cw, P)
    assert np.array_equal(inter, e_inter) and np.array_equal(area, e_area)
    assert not area[1].any() and not inter[1].any() and not inter[2, 0].any()  # the all-background frame, as current and as past
    assert not inter[0, 3].any() and (P == 1 or inter[0, :3].any())  # lag 4 of frame 0 reaches slot 0, which is not valid
    for n_hist in (2, 4):
        inter, area = run(second, ring, n_hist, rw, cw, P, nbytes)
        e_inter, e_area = brute_fast(second, ring, n_hist, rw, cw, P)
        assert np.array_equal(inter, e_inter) and np.array_equal(area, e_area)


def test_mask_pairs_identical_across_runs_and_streams():
    g = np.random.default_rng(7)
    rw, cw = weights(g)
    cur, hist = random_maps(g, B, 5), random_maps(g, L, 5)
    a = run(cur, hist, 4, rw, cw, 5, 1)
    b = run(cur, hist, 4, rw, cw, 5, 1)
    c = run(cur, hist, 4, rw, cw, 5, 1, stream=torch.cuda.Stream(DEV))
    for x, y in ((a, b), (a, c)):
        assert np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1])


def test_mask_pairs_rejects_bad_arguments():
    from sleap_nn_amd import _lib as L_

    lib = L_.lib()
    t = torch.zeros(1 << 16, dtype=torch.int32, device=DEV)
    p = C.c_void_p(t.data_ptr())
    at = lambda k: C.c_void_p(t.data_ptr() + 4 * 4096 * k)  # inputs and outputs apart
    base = dict(labels=p, nbytes=1, B=2, h=8, w=8, hist=at(1), L=2, n_hist=1, rw=at(2), cw=at(3), px=64, P=4, inter=at(4), area=at(5))
    call = lambda **kw: lib.ph_track_mask_pairs(*[{**base, **kw}[k] for k in ("labels", "nbytes", "B", "h", "w", "hist", "L", "n_hist", "rw", "cw", "px", "P", "inter", "area")], None)
    assert call() == L_.PH_OK
    torch.cuda.synchronize()
    for bad in (dict(labels=None), dict(hist=None), dict(rw=None), dict(cw=None), dict(inter=None), dict(area=None), dict(nbytes=3), dict(nbytes=8), dict(B=0), dict(h=0),
                dict(w=0), dict(L=0), dict(L=33), dict(n_hist=3), dict(n_hist=-1), dict(P=0), dict(P=65), dict(px=2**31), dict(px=-1)):
        assert call(**bad) == L_.PH_E_INVALID, bad
    assert b"image pixels" in lib.ph_last_error()


# ---- end to end -----------------------------------------------------------------------------------------------------

def head_maps(n_frames=7, hw=(40, 48), stride=2, seed=11):
    """Synthetic head maps: three discs on slow paths (one leaves for a frame), foreground probability 0.95 inside, a Gaussian centre map and offsets that point
    from every pixel to its disc's centre."""
    g = np.random.default_rng(seed)
    h, w = hw
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    pos = np.array([[10.0, 10.0], [34.0, 12.0], [22.0, 28.0]])
    vel = np.array([[1.2, 0.8], [-1.0, 0.9], [0.6, -1.1]])
    fg = np.full((n_frames, 1, h, w), 0.02, dtype=np.float32)
    hm = np.zeros((n_frames, 1, h, w), dtype=np.float32)
    off = np.zeros((n_frames, 2, h, w), dtype=np.float32)
    for t in range(n_frames):
        pos = pos + vel + g.normal(0, 0.2, pos.shape)
        for a in range(3):
            if a == 2 and t == 3:
                continue
            cx, cy = np.round(pos[a])
            inside = (xx - cx) ** 2 + (yy - cy) ** 2 <= 5.0**2
            fg[t, 0][inside] = 0.95
            hm[t, 0] = np.maximum(hm[t, 0], 0.9 * np.exp(-((xx - cx) ** 2 + (yy - cy) ** 2) / (2 * 1.5**2)))
            off[t, 0][inside] = ((cx - xx) * stride)[inside]
            off[t, 1][inside] = ((cy - yy) * stride)[inside]
    return fg, hm, off


@pytest.mark.parametrize("full_res", [False, True])
def test_device_tables_track_like_host_scoring(full_res):
    from sleap_nn_amd.inference.layers.segmentation import SegmentationLayer
    from sleap_nn_amd.inference.preprocess_info import PreprocInfo
    from sleap_nn_amd.tracking import Tracker
    from tests.test_segmentation_cpu import StubBackend

    stride = 2
    fg, hm, off = head_maps(stride=stride)
    layer = SegmentationLayer(StubBackend(), stride, full_res_masks=full_res, keep_label_map=True)
    plain = SegmentationLayer(StubBackend(), stride, full_res_masks=full_res)
    kw = dict(features="masks", scoring_method="mask_iou", window_size=4)
    dev_tr, host_tr, frame_tr = Tracker.from_config(**kw), Tracker.from_config(**kw), Tracker.from_config(**kw)
    per_frame, lifetimes = [], {}
    t0 = 0
    for n in (3, 3, 1):
        sl = slice(t0, t0 + n)
        info = PreprocInfo(original_size=(75, 93), processed_size=(80, 96), eff_scale=torch.ones(n), input_scale=1.0, output_stride=stride)  # valid 38 x 47 of 40 x 48 cells
        raw = {"SegmentationHead": torch.from_numpy(fg[sl]).to(DEV), "InstanceCenterHead": torch.from_numpy(hm[sl]).to(DEV), "CenterOffsetHead": torch.from_numpy(off[sl]).to(DEV)}
        out = layer.postprocess(raw, info)
        out.frame_indices = torch.arange(t0, t0 + n)
        assert out.pred_label_map is not None and out.pred_label_map.is_cuda and len(out.pred_mask_labels) == n
        rw, cw = out.pred_label_weights[0]
        assert rw.sum() == 75 and cw.sum() == 93 and (rw[38:] == 0).all() and (cw[47:] == 0).all()
        base = plain.postprocess(raw, info)
        assert base.pred_label_map is None and base.pred_mask_labels is None  # without the flag nothing is added
        assert all(np.array_equal(a["mask"], b["mask"]) for fa, fb in zip(out.pred_masks, base.pred_masks) for a, b in zip(fa, fb))
        a = dev_tr.track_outputs(out)
        b = host_tr.track_outputs(out, use_tables=False)
        for k in range(n):
            ids = [m["track_id"] for m in a.pred_masks[k]]
            assert ids == [m["track_id"] for m in b.pred_masks[k]]
            sa, sb = [m["tracking_score"] for m in a.pred_masks[k]], [m["tracking_score"] for m in b.pred_masks[k]]
            assert np.array_equal(np.array(sa), np.array(sb), equal_nan=True)  # bit-equal
            f_ids, f_sc = frame_tr.track(out.pred_masks[k], t0 + k)
            assert ids == f_ids.tolist() and np.array_equal(np.array(sa), f_sc, equal_nan=True)
            per_frame.append(len(ids))
            for i in ids:
                lifetimes[i] = lifetimes.get(i, 0) + 1
        t0 += n
    # not vacuous
    assert sum(c >= 2 for c in per_frame) >= 3 and max(lifetimes.values()) >= 3
    assert dev_tr.table_hits > 0 and dev_tr.pair_calls == 0 and host_tr.table_hits == 0 and host_tr.pair_calls > 0


def test_run_directory_with_tracker_through_predictor():
    from sleap_nn_amd.inference.predictor import Predictor
    from sleap_nn_amd.tracking import TrackerConfig

    seg = G.load("segmentation.npz")
    path = [os.path.join(G.GOLDEN_DIR, "ckpt_dirs", "tiny_bottomup_segmentation")]
    f = seg["rundir/frames"]
    frames = np.stack([f[0], f[0], f[0], f[1]])  # 4 frames in 2 batches: the first frame three times (in one batch, and across the ring), then another
    cfg = TrackerConfig(scoring_method_explicit=False, features_explicit=False, candidates_method_explicit=False)
    tracked = Predictor.from_model_paths(path, device=DEV, batch_size=2, tracker_config=cfg)
    plain = Predictor.from_model_paths(path, device=DEV, batch_size=2, tracker_config=None)
    assert tracked.layer.keep_label_map and not plain.layer.keep_label_map
    a, b = tracked.predict(frames), plain.predict(frames)
    assert len(a) == len(b) == 2
    ids = []
    for oa, ob in zip(a, b):
        assert ob.pred_label_map is None and ob.pred_mask_labels is None and ob.instance_track_ids is None and oa.pred_label_map is not None
        for fa, fb in zip(oa.pred_masks, ob.pred_masks):
            assert len(fa) == len(fb) >= 2
            for ma, mb in zip(fa, fb):
                assert "track_id" not in mb and set(ma) == set(mb) | {"track_id", "tracking_score"}
                assert np.array_equal(ma["mask"], mb["mask"]) and ma["score"] == mb["score"] and ma["scale"] == mb["scale"]
            ids.append([m["track_id"] for m in fa])
    assert all(i >= 0 for f in ids for i in f) and len(set(ids[0])) == len(ids[0])
    # the same frame again: every mask meets itself with IoU 1 and the frame's other masks (disjoint) with IoU 0, inside the batch and from the ring
    assert ids[1] == ids[0] and ids[2] == ids[0]
    assert all(m["tracking_score"] == 1.0 for fr in (a[0].pred_masks[1], a[1].pred_masks[0]) for m in fr)
