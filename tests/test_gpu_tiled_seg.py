"""Tiled segmentation inference on the GPU: ``ph_tile_merge_heads`` bit for bit against the torch ``TileMerger`` canvas, ``merge_tiles`` per head and the
reference's recorded merges; ``TiledSegmentationLayer`` / ``TiledSemanticSegmentationLayer`` on the device with the reference's recorded tile maps and end to
end with ``HipBackend`` through the predictor (tests/golden/tiled_segmentation.npz, tools/gen_tiled_seg_golden.py)."""
import ctypes as C
import json
import os
import shutil

import numpy as np
import pytest
import torch
import yaml

from tests import _golden as G
from tests import _tiled_seg as TS

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BLENDS = ("gaussian", "pyramid", "constant")
HEAD_ATOL = 1e-4  # the project's parity bound for head outputs against the reference's CPU forward (tests/test_gpu_parity.py); the stitch is a weighted mean
HEADS = {"fg_cen_off": (1, 1, 2), "one_head": (1,)}

# name -> (F, th = tw, y origins, x origins, (h, w))
MERGE_SHAPES = {
    "single_pixel_45x67": (2, 16, [0, 13, 29], [0, 13, 26, 39, 51], (45, 67)),  # odd width: one pixel per thread (67 columns need 5 tiles of 16)
    "vector_cut_groups_44x68": (2, 16, [0, 14, 28], [0, 13, 26, 39, 52], (44, 68)),  # w % 4 == 0, x origins that cut groups of 4 (68 columns need 5 tiles of 16)
    "frame_smaller_than_a_tile_scalar": (1, 16, [0], [0], (10, 13)),
    "frame_smaller_than_a_tile_vector": (2, 16, [0], [0], (9, 12)),
}


def _torch_canvas(tiles, window, ys, xs, hw, frames):
    """One ``TileMerger`` canvas of all channels per frame, the way the reference's layer drives it: canvas max(frame, tile), crop."""
    from sleap_nn_amd.inference.tile_merger import TileMerger

    h, w = hw
    T = len(ys) * len(xs)
    th, tw = tiles.shape[-2:]
    out = []
    for f in range(frames):
        m = TileMerger((max(h, th), max(w, tw)), tiles.shape[1], window)
        for k, (y0, x0) in enumerate((y0, x0) for y0 in ys for x0 in xs):
            m.integrate(tiles[f * T + k], y0, x0)
        out.append(m.merge()[:, :h, :w])
    return torch.stack(out)


def _random_tiles(n, c, t, seed):
    g = torch.Generator().manual_seed(seed)
    tiles = torch.randn((n, c, t, t), generator=g)
    tiles[:, 0] = torch.rand((n, t, t), generator=g)  # a probability-like channel
    return tiles


def _split(tiles, channels):
    return [a.contiguous() for a in torch.split(tiles, list(channels), dim=1)]


# ---- ph_tile_merge_heads ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", BLENDS)
@pytest.mark.parametrize("heads", list(HEADS))
@pytest.mark.parametrize("shape", list(MERGE_SHAPES))
def test_merge_heads_is_bit_identical_to_the_torch_canvas_and_to_merge_tiles(shape, heads, mode):
    from sleap_nn_amd.inference.tile_merger import build_importance_window, merge_tile_heads, merge_tiles

    F, t, ys, xs, hw = MERGE_SHAPES[shape]
    channels = HEADS[heads]
    tiles = _random_tiles(F * len(ys) * len(xs), sum(channels), t, seed=len(shape) * 10 + len(channels))
    win = build_importance_window((t, t), mode=mode)
    want = _torch_canvas(tiles, win, ys, xs, hw, F)
    assert not torch.isnan(want).any()
    arenas = [a.to(DEV) for a in _split(tiles, channels)]
    got = merge_tile_heads(arenas, win, ys, xs, hw, frames=F)
    assert len(got) == len(channels)
    for g, a, wpart, c in zip(got, arenas, torch.split(want, list(channels), dim=1), channels):
        assert tuple(g.shape) == (F, c) + tuple(hw) and g.is_contiguous() and g.dtype == torch.float32
        same = TS.bits(g) == TS.bits(wpart)
        assert same.all(), (shape, heads, mode, int((~same).sum()), np.argwhere(~same)[:4].tolist())
        assert np.array_equal(TS.bits(g), TS.bits(merge_tiles(a, win, ys, xs, hw, frames=F)))


@pytest.mark.parametrize("channels", [(2, 1), (1, 1, 1, 1), (3, 2), (2, 2, 2), (4, 3), (8,), (2, 2, 2, 2)], ids=str)
def test_every_total_channel_count_and_head_count(channels):
    from sleap_nn_amd.inference.tile_merger import build_importance_window, merge_tile_heads

    ys, xs, t, hw, F = [0, 10], [0, 12, 20], 16, (26, 36), 2
    tiles = _random_tiles(F * 6, sum(channels), t, seed=sum(channels) * 7 + len(channels))
    win = build_importance_window((t, t))
    want = _torch_canvas(tiles, win, ys, xs, hw, F)
    got = merge_tile_heads([a.to(DEV) for a in _split(tiles, channels)], win.to(DEV), ys, xs, hw, frames=F)
    assert np.array_equal(TS.bits(torch.cat(got, dim=1)), TS.bits(want))


def test_uncovered_pixels_are_nan_where_the_torch_merger_has_them():
    from sleap_nn_amd.inference.tile_merger import build_importance_window, merge_tile_heads

    ys, xs, t = [0], [0, 40], 16  # rows 16.. and columns 16..39, 56.. are covered by no tile
    tiles = _random_tiles(2, 4, t, seed=4).abs() + 0.5
    win = build_importance_window((t, t), mode="pyramid")
    for hw in ((20, 60), (20, 59)):  # vector and scalar path
        want = _torch_canvas(tiles, win, ys, xs, hw, 1)
        nan = torch.isnan(want).numpy()
        assert nan.any() and not nan.all()
        got = torch.cat(merge_tile_heads([a.to(DEV) for a in _split(tiles, (1, 1, 2))], win, ys, xs, hw), dim=1).cpu()
        assert np.array_equal(torch.isnan(got).numpy(), nan)
        assert np.array_equal(TS.bits(got)[~nan], TS.bits(want)[~nan])


def test_an_output_that_is_not_16_byte_aligned_takes_the_single_pixel_path():
    from sleap_nn_amd.inference.tile_merger import build_importance_window, merge_tile_heads_into, origins_tensor

    F, t, ys, xs, (h, w) = MERGE_SHAPES["vector_cut_groups_44x68"]
    channels = (1, 1, 2)
    tiles = _random_tiles(F * len(ys) * len(xs), 4, t, seed=11)
    win = build_importance_window((t, t))
    want = torch.split(_torch_canvas(tiles, win, ys, xs, (h, w), F), list(channels), dim=1)
    arenas = [a.to(DEV) for a in _split(tiles, channels)]
    for shift in ((0, 1, 0), (3, 0, 2)):  # one unaligned output is enough to leave the 16-byte path
        bases = [torch.full((F * c * h * w + 8,), 7.0, device=DEV) for c in channels]
        outs = [b[s : s + F * c * h * w].view(F, c, h, w) for b, s, c in zip(bases, shift, channels)]
        assert [o.data_ptr() % 16 for o in outs] == [4 * s for s in shift]
        merge_tile_heads_into(arenas, win.to(DEV), origins_tensor(ys, DEV), origins_tensor(xs, DEV), outs)
        for o, wp, b, s, c in zip(outs, want, bases, shift, channels):
            assert np.array_equal(TS.bits(o), TS.bits(wp))
            assert (b[:s] == 7.0).all() and (b[s + F * c * h * w :] == 7.0).all()  # nothing written outside the view


def test_recorded_reference_merger_cases_bit_for_bit():
    from sleap_nn_amd.inference.tile_merger import build_importance_window, merge_tile_heads

    z = TS.golden()
    names = json.loads(str(z["merger/names"]))
    assert names == ["odd", "vec"]
    for name in names:
        p = json.loads(str(z[f"merger/{name}/params"]))
        tiles = torch.from_numpy(z[f"merger/{name}/tiles"])
        win = build_importance_window((p["tile"], p["tile"]), mode=p["blend"])
        for channels in ((1, 1, 2), (4,)):
            got = merge_tile_heads([a.to(DEV) for a in _split(tiles, channels)], win, p["ys"], p["xs"], tuple(p["hw"]))
            assert np.array_equal(TS.bits(torch.cat(got, dim=1)[0]), TS.bits(z[f"merger/{name}/merged"])), (name, channels)


def test_non_default_stream_and_repeatability():
    from sleap_nn_amd.inference.tile_merger import build_importance_window, merge_tile_heads

    F, t, ys, xs, hw = MERGE_SHAPES["vector_cut_groups_44x68"]
    tiles = _random_tiles(F * len(ys) * len(xs), 4, t, seed=21)
    win = build_importance_window((t, t)).to(DEV)
    arenas = [a.to(DEV) for a in _split(tiles, (1, 1, 2))]
    first = torch.cat(merge_tile_heads(arenas, win, ys, xs, hw, frames=F), dim=1)
    torch.cuda.synchronize()
    st = torch.cuda.Stream(DEV)
    with torch.cuda.stream(st):
        runs = [torch.cat(merge_tile_heads(arenas, win, ys, xs, hw, frames=F), dim=1) for _ in range(3)]
    st.synchronize()
    for r in runs:
        assert np.array_equal(TS.bits(r), TS.bits(first))
    assert np.array_equal(TS.bits(first), TS.bits(_torch_canvas(tiles, win.cpu(), ys, xs, hw, F)))


def test_bad_arguments_are_rejected():
    from sleap_nn_amd import _lib as L
    from sleap_nn_amd.inference.tile_merger import build_importance_window, merge_tile_heads

    lib = L.lib()
    F, t, ny, nx, h, w = 1, 16, 2, 2, 24, 24
    arenas = [torch.zeros((F * ny * nx, c, t, t), device=DEV) for c in (1, 1, 2, 3, 3)]
    outs = [torch.zeros((F, c, h, w), device=DEV) for c in (1, 1, 2, 3, 3)]
    win = torch.ones((t, t), device=DEV)
    o = torch.tensor([0, 8], dtype=torch.int32, device=DEV)
    s = L.current_stream_ptr()
    P = lambda x: C.c_void_p(x.data_ptr())

    def call(a, ch, o_, K=None, win_=win, F_=F, th=t, tw=t, ny_=ny, nx_=nx, h_=h, w_=w):
        K = len(a) if K is None else K
        n = max(len(a), 1)
        ap = (C.c_void_p * n)(*[x if x is None or isinstance(x, int) else x.data_ptr() for x in a])
        op = (C.c_void_p * n)(*[x if x is None or isinstance(x, int) else x.data_ptr() for x in o_])
        cp = (C.c_int32 * n)(*ch)
        rc = lib.ph_tile_merge_heads(ap, cp, K, None if win_ is None else P(win_), F_, th, tw, P(o), ny_, P(o), nx_, h_, w_, op, s)
        return rc, lib.ph_last_error().decode()

    def rejected(match, *a, **k):
        rc, msg = call(*a, **k)
        assert rc == L.PH_E_INVALID and msg.startswith("ph_tile_merge_heads:") and match in msg, (rc, msg)

    ok3, out3, ch3 = arenas[:3], outs[:3], (1, 1, 2)
    assert call(ok3, ch3, out3)[0] == L.PH_OK
    rejected("null pointer", ok3, ch3, out3, win_=None)
    rejected("null pointer", [arenas[0], None, arenas[2]], ch3, out3)
    rejected("null pointer", ok3, ch3, [outs[0], outs[1], None])
    rejected("K must be", ok3, ch3, out3, K=0)
    rejected("K must be", arenas, (1, 1, 2, 3, 3), outs, K=5)
    rejected("channels", ok3, (1, 0, 2), out3)
    rejected("channels", ok3[:1], (9,), out3[:1])
    rejected("channels in total", [arenas[2], arenas[3], arenas[4], arenas[0]], (2, 3, 3, 1), [outs[2], outs[3], outs[4], outs[0]])
    rejected("bad tile-map shape", ok3, ch3, out3, F_=0)
    rejected("bad tile-map shape", ok3, ch3, out3, tw=0)
    rejected("bad grid / output", ok3, ch3, out3, ny_=0)
    rejected("bad grid / output", ok3, ch3, out3, w_=-4)
    rejected("too many tiles", ok3, ch3, out3, F_=65536, ny_=256, nx_=256)
    rejected("aliases arena", ok3, ch3, [outs[0], arenas[2], outs[2]])  # an output that is an arena
    rejected("aliases arena", ok3, ch3, [outs[0], outs[1], arenas[0].data_ptr() + 64])  # ... or starts inside one
    rejected("aliases output", ok3, ch3, [outs[0], outs[0], outs[2]])
    rejected("aliases output", ok3, ch3, [outs[3], outs[1], outs[3].data_ptr() + 2 * h * w])  # overlapping byte ranges of one buffer
    torch.cuda.synchronize()

    # the wrapper's own checks
    wn = build_importance_window((t, t))
    with pytest.raises(RuntimeError):
        merge_tile_heads([arenas[0].cpu()], wn, [0, 8], [0, 8], (h, w))
    for bad in ([], arenas, [arenas[2], arenas[3], arenas[4], arenas[0]], [arenas[0].double()], [arenas[0][0]], [arenas[0], arenas[1][:2]],
                [arenas[0], torch.zeros((4, 1, 8, 8), device=DEV)]):
        with pytest.raises(ValueError):
            merge_tile_heads(bad, wn, [0, 8], [0, 8], (h, w))
    with pytest.raises(ValueError):
        merge_tile_heads(ok3, wn, [0, 8], [0, 8], (h, w), frames=2)
    with pytest.raises(ValueError):
        merge_tile_heads(ok3, wn[:8], [0, 8], [0, 8], (h, w))
    with pytest.raises(ValueError):
        merge_tile_heads(ok3, wn, [], [0, 8], (h, w))


# ---- the layers on the device, fed the reference's recorded tile maps ---------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,name", TS.ALL_CASES, ids=[f"{k}-{n}" for k, n in TS.ALL_CASES])
def test_layers_reproduce_the_reference_from_its_recorded_tile_maps(kind, name):
    c = TS.Case(kind, name)
    be = TS.ReplayBackend(c, DEV)
    layer = TS.tiled_layer(c, be)
    seen = TS.spy_postprocess(layer)
    out = layer.predict(torch.from_numpy(c.frames))
    assert len(seen) == 1
    raw_out, info = seen[0]
    assert np.array_equal(TS.bits(TS.stitched_of(c, raw_out)), TS.bits(c.stitched))
    assert tuple(info.processed_size) == tuple(c.frames.shape[-2:]) and info.output_stride == 2 and info.eff_scale.numel() == c.F
    assert max(be.batch_sizes) <= c.params["tile_batch_size"] and sum(be.batch_sizes) == c.F * c.T
    TS.check_entries(c, out.pred_masks, tag=f"{kind}/{name}")


@pytest.mark.parametrize("kind,name", [("bu", "t64"), ("bu", "tiny"), ("sem", "t32")])
def test_host_accumulator_equals_the_kernel_bit_for_bit(kind, name):
    c = TS.Case(kind, name)
    got = {}
    for acc in ("cuda", "cpu", "auto"):
        layer = TS.tiled_layer(c, TS.ReplayBackend(c, DEV), accumulator_device=acc)
        seen = TS.spy_postprocess(layer)
        out = layer.predict(torch.from_numpy(c.frames))
        got[acc] = (TS.stitched_of(c, seen[0][0]), out.pred_masks)
    for acc in ("cpu", "auto"):
        assert np.array_equal(TS.bits(got[acc][0]), TS.bits(got["cuda"][0])), acc
        for fa, fb in zip(got[acc][1], got["cuda"][1]):
            assert len(fa) == len(fb) and all(np.array_equal(a["mask"], b["mask"]) and a["score"] == b["score"] for a, b in zip(fa, fb))
    assert np.array_equal(TS.bits(got["cpu"][0]), TS.bits(c.stitched))


def test_tile_batch_size_bounds_every_backend_call():
    c = TS.Case("bu", "t64")
    for tbs, want in ((1, [1] * 12), (5, [5, 5, 2]), (8, [8, 4]), (64, [12])):
        be = TS.ReplayBackend(c, DEV)
        out = TS.tiled_layer(c, be, tile_batch_size=tbs).predict(torch.from_numpy(c.frames))
        assert be.batch_sizes == want, (tbs, be.batch_sizes)
        TS.check_entries(c, out.pred_masks, tag=f"tbs{tbs}")


# ---- end to end -----------------------------------------------------------------------------------------------------------------------------------------
def _run_dir_with_tiling(tmp_path, kind, tiling):
    dst = tmp_path / kind
    shutil.copytree(os.path.join(G.GOLDEN_DIR, "ckpt_dirs", kind), dst)
    cfg = yaml.safe_load(open(dst / "training_config.yaml"))
    cfg["data_config"]["preprocessing"]["tiling"] = tiling
    with open(dst / "training_config.yaml", "w") as f:
        yaml.safe_dump(cfg, f)
    return str(dst)


def _tiling_of(c):
    p = c.params
    return {"enabled": True, "tile_size": p["tile_size"], "overlap": p["overlap"], "blend": p["blend"], "tile_batch_size": p["tile_batch_size"]}


@pytest.mark.parametrize("kind,name", [("bu", "t64"), ("bu", "t32"), ("bu", "tiny"), ("sem", "t64"), ("sem", "t32")])
def test_run_directory_end_to_end_through_the_predictor(tmp_path, kind, name):
    from sleap_nn_amd.inference.layers import SegmentationLayer, SemanticSegmentationLayer, TiledSegmentationLayer, TiledSemanticSegmentationLayer
    from sleap_nn_amd.inference.predictor import Predictor

    c = TS.Case(kind, name)
    run = "tiny_tiled_semantic_segmentation" if c.semantic else "tiny_bottomup_segmentation"
    d = _run_dir_with_tiling(tmp_path, run, _tiling_of(c))
    with pytest.raises(NotImplementedError, match="tiled_segmentation=True"):
        Predictor.from_model_paths([d], device=DEV)
    pred = Predictor.from_model_paths([d], device=DEV, batch_size=2, tiled_segmentation=True, tile_size=c.params["tile_size"], overlap=c.params["overlap"],
                                      fg_threshold=c.params["fg_threshold"], peak_threshold=c.params["peak_threshold"])
    layer = pred.layer
    assert type(layer) is (TiledSemanticSegmentationLayer if c.semantic else TiledSegmentationLayer) and pred.replicas == []
    assert type(layer.inner) is (SemanticSegmentationLayer if c.semantic else SegmentationLayer)
    assert (layer.tile_size, layer.overlap, layer._blend, layer.tile_batch_size) == (c.params["tile_size"], c.params["overlap"], c.params["blend"], c.params["tile_batch_size"])
    seen = TS.spy_postprocess(layer)
    outs = pred.predict(c.frames)
    assert len(outs) == 1 and len(seen) == 1 and outs[0].frame_indices.tolist() == list(range(c.F))
    got = TS.stitched_of(c, seen[0][0])
    err = np.abs(got - c.stitched).reshape(c.F, got.shape[1], -1).max(-1)
    print(f"{kind}/{name}: stitched heads max |d| per frame and channel against the reference's {err.tolist()}")
    assert got.shape == c.stitched.shape and err.max() <= HEAD_ATOL, (kind, name, float(err.max()))
    TS.check_entries(c, outs[0].pred_masks, tag=f"e2e {kind}/{name}")


def test_tiled_bottom_up_predictor_with_a_tracker(tmp_path):
    from sleap_nn_amd.inference.predictor import Predictor
    from sleap_nn_amd.tracking import TrackerConfig, apply_tracking

    c = TS.Case("bu", "t64")
    d = _run_dir_with_tiling(tmp_path, "tiny_bottomup_segmentation", _tiling_of(c))
    cfg = TrackerConfig(scoring_method_explicit=False, features_explicit=False, candidates_method_explicit=False)
    tracked = Predictor.from_model_paths([d], device=DEV, batch_size=2, tiled_segmentation=True, tracker_config=cfg)
    plain = Predictor.from_model_paths([d], device=DEV, batch_size=2, tiled_segmentation=True)
    assert tracked.layer.inner.keep_label_map and not plain.layer.inner.keep_label_map
    frames = np.stack([c.frames[0], c.frames[0], c.frames[1], c.frames[0]])  # two batches
    a, b = tracked.predict(frames), plain.predict(frames)
    host = apply_tracking(b, cfg, use_tables=False)  # the same tracker on the host masks alone
    assert len(a) == len(b) == 2
    for oa, ob, oh in zip(a, b, host):
        assert ob.pred_label_map is None and ob.pred_mask_labels is None
        assert oa.pred_label_map is not None and oa.pred_label_map.is_cuda and tuple(oa.pred_label_map.shape) == (2, 45, 67)
        assert len(oa.pred_mask_labels) == 2 and len(oa.pred_label_weights) == 2
        rw, cw = oa.pred_label_weights[0]
        assert rw.sum() == 90 and cw.sum() == 134
        for fa, fb, fh, labels in zip(oa.pred_masks, ob.pred_masks, oh.pred_masks, oa.pred_mask_labels):
            assert len(fa) == len(fb) == len(fh) == len(labels) >= 2
            assert all(np.array_equal(ma["mask"], mb["mask"]) for ma, mb in zip(fa, fb))
            assert [m["track_id"] for m in fa] == [m["track_id"] for m in fh]
    ids = [[m["track_id"] for m in f] for o in a for f in o.pred_masks]
    assert ids[1] == ids[0] and all(i >= 0 for f in ids for i in f)  # the same frame again: every mask meets itself
