"""Tiled single-instance inference on the GPU: ``ph_tile_extract`` against torch slicing, ``ph_tile_merge`` bit for bit against the
reference's recorded ``TileMerger`` results and the in-repo torch ``TileMerger``, and ``TiledLayer`` / ``Predictor`` on the fixture
checkpoint against the reference's own ``TiledLayer`` run (tests/golden/tiling.npz, tools/gen_tiling_golden.py)."""
import json
import os
import shutil

import numpy as np
import pytest
import torch
import yaml

from tests import _golden as G

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BLENDS = ("gaussian", "pyramid", "constant")
CMS_ATOL = 1e-4  # the project's bar against the reference's CPU path (tests/test_gpu_parity.py); the stitch adds no error of its own
KPT_ATOL = 1e-3
RUN_DIR = os.path.join(G.GOLDEN_DIR, "ckpt_dirs", "minimal_instance_single_instance")


@pytest.fixture(scope="module")
def z():
    return G.load("tiling.npz")


def _bits(t):
    if torch.is_tensor(t):
        t = t.detach().cpu().numpy()
    return np.ascontiguousarray(t, dtype=np.float32).view(np.int32)


# ---- ph_tile_extract -------------------------------------------------------------------------------------------------------------
def _slice_tiles(frames, ys, xs, ts):
    """The reference's ``_extract_square_tile`` per tile, row-major per frame, on the host."""
    F, C, H, W = frames.shape
    out = []
    for f in range(F):
        for y0 in ys:
            for x0 in xs:
                tile = frames.new_zeros((C, ts, ts))
                ye, xe = min(H, y0 + ts), min(W, x0 + ts)
                if ye > y0 and xe > x0:
                    tile[:, : ye - y0, : xe - x0] = frames[f, :, y0:ye, x0:xe]
                out.append(tile)
    return torch.stack(out)


EXTRACT_CASES = [
    # F, C, H, W, tile, y origins, x origins
    (1, 1, 64, 96, 32, [0, 16, 32], [0, 32, 64]),  # aligned rows and origins
    (2, 3, 45, 77, 32, [0, 13], [0, 5, 18, 45]),  # odd width, origins that leave rows unaligned (also for 4-byte loads)
    (2, 3, 45, 77, 32, [0, 12], [0, 4, 20, 44]),  # 4-byte-aligned origins on an odd width
    (3, 1, 50, 70, 20, [0, 8, 30], [0, 6, 50]),  # tile side not a multiple of 16
    (2, 3, 40, 52, 64, [0], [0]),  # frame smaller than the tile: zero padded
    (1, 2, 40, 100, 64, [0], [0, 36]),  # smaller on one axis only
    (1, 1, 33, 47, 16, [20, 30], [40, 44]),  # tiles that run over the bottom / right edge
    (2, 3, 1500, 1700, 512, [0, 494, 988], [0, 594, 1188]),  # more chunks than one pass of the grid: the grid-stride loop runs
]


@pytest.mark.parametrize("dtype", [torch.uint8, torch.float32])
@pytest.mark.parametrize("case", EXTRACT_CASES, ids=lambda c: f"F{c[0]}C{c[1]}_{c[2]}x{c[3]}_t{c[4]}")
def test_tile_extract_equals_torch_slicing(case, dtype):
    from sleap_nn_amd.inference.tile_merger import extract_tiles

    F, C, H, W, ts, ys, xs = case
    g = torch.Generator().manual_seed(H * 1000 + W)
    frames = torch.randint(1, 256, (F, C, H, W), dtype=torch.uint8, generator=g)  # (no zeros: a missing pixel cannot pass for padding)
    if dtype == torch.float32:
        frames = frames.float() / 7.0
    got = extract_tiles(frames.to(DEV), ys, xs, ts)
    want = _slice_tiles(frames, ys, xs, ts)
    assert got.dtype == dtype and tuple(got.shape) == (F * len(ys) * len(xs), C, ts, ts)
    assert torch.equal(got.cpu(), want)


def test_tile_extract_from_an_unaligned_view_and_bad_arguments():
    import ctypes as C

    from sleap_nn_amd import _lib as L
    from sleap_nn_amd.inference.tile_merger import extract_tiles

    g = torch.Generator().manual_seed(5)
    base = torch.randint(1, 256, (1 + 2 * 3 * 40 * 64,), dtype=torch.uint8, generator=g)
    frames = base[1:].view(2, 3, 40, 64)  # contiguous, but the storage starts one byte past an aligned address
    dev = base.to(DEV)[1:].view(2, 3, 40, 64)
    assert dev.data_ptr() % 4 == 1
    assert torch.equal(extract_tiles(dev, [0, 8], [0, 16, 32], 32).cpu(), _slice_tiles(frames, [0, 8], [0, 16, 32], 32))
    with pytest.raises(ValueError):
        extract_tiles(dev.to(torch.int16), [0], [0], 32)
    with pytest.raises(ValueError):
        extract_tiles(dev, [], [0], 32)
    with pytest.raises(RuntimeError):
        extract_tiles(frames, [0], [0], 32)  # host tensor
    lib, P = L.lib(), lambda t: C.c_void_p(t.data_ptr())
    o = torch.zeros(2, dtype=torch.int32, device=DEV)
    out = torch.empty((2, 3, 32, 32), dtype=torch.uint8, device=DEV)
    s = L.current_stream_ptr()
    assert lib.ph_tile_extract(None, 0, 2, 3, 40, 64, P(o), 1, P(o), 1, 32, P(out), s) == L.PH_E_INVALID
    assert lib.ph_tile_extract(P(dev), 2, 2, 3, 40, 64, P(o), 1, P(o), 1, 32, P(out), s) == L.PH_E_INVALID
    assert lib.ph_tile_extract(P(dev), 0, 2, 3, 40, 64, P(o), 0, P(o), 1, 32, P(out), s) == L.PH_E_INVALID
    assert lib.ph_tile_extract(P(dev), 0, 2, 3, 40, 64, P(o), 1, P(o), 1, 0, P(out), s) == L.PH_E_INVALID


# ---- ph_tile_merge ---------------------------------------------------------------------------------------------------------------
def _torch_merge(tiles, window, ys, xs, hw, frames=1):
    """The in-repo torch ``TileMerger`` on the host, the way the reference's layer drives it: canvas max(frame, tile), crop."""
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


def test_tile_merge_is_bit_identical_to_the_recorded_reference_merges(z):
    from sleap_nn_amd.inference.tile_merger import merge_tiles

    names = json.loads(str(z["merge/names"]))
    assert len(names) >= 5
    for name in names:
        tiles = torch.from_numpy(z[f"merge/{name}/tiles"]).to(DEV)
        ys, xs = z[f"merge/{name}/y_origins"].tolist(), z[f"merge/{name}/x_origins"].tolist()
        h, w = z[f"merge/{name}/out_hw"].tolist()
        for mode in BLENDS:
            win = torch.from_numpy(z[f"merge/{name}/{mode}/window"])
            got = merge_tiles(tiles, win, ys, xs, (h, w))
            want = z[f"merge/{name}/{mode}/merged"]
            assert tuple(got.shape) == (1,) + want.shape
            same = _bits(got[0]) == _bits(want)
            assert same.all(), (name, mode, int((~same).sum()), np.argwhere(~same)[:4].tolist())


# (N, th = tw, y origins, x origins, (h, w)): more output pixels than one pass of the grid holds (8 workgroups of 256 threads per CU, 4 pixels
# per thread on the vector path, 1 on the scalar one), non-square, origins that are and are not multiples of 4
BIG_MERGES = {
    "vector_path": (2, 256, [0, 200, 420, 650, 844], [0, 190, 381, 570, 760, 950, 1140, 1330, 1520, 1710, 1796], (1100, 2052)),
    "scalar_path_odd_width": (2, 128, [0, 96, 190, 290, 380, 472], [0, 97, 194, 291, 388, 485, 582, 679, 776, 873], (600, 1001)),
}


@pytest.mark.parametrize("mode", BLENDS)
@pytest.mark.parametrize("name", list(BIG_MERGES))
def test_tile_merge_is_bit_identical_to_the_torch_merger_on_large_frames(name, mode):
    from sleap_nn_amd.inference.tile_merger import build_importance_window, merge_tiles

    N, t, ys, xs, (h, w) = BIG_MERGES[name]
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert h * w > 2 * cus * 256 and h * w > cus * 8 * 256 * (4 if w % 4 == 0 else 1)
    g = torch.Generator().manual_seed(len(name))
    tiles = torch.randn((len(ys) * len(xs), N, t, t), generator=g)
    tiles[:, 1] = torch.rand((len(ys) * len(xs), t, t), generator=g)
    win = build_importance_window((t, t), mode=mode)
    got = merge_tiles(tiles.to(DEV), win, ys, xs, (h, w))
    want = _torch_merge(tiles, win, ys, xs, (h, w))
    assert not torch.isnan(want).any()
    same = _bits(got) == _bits(want)
    assert same.all(), (int((~same).sum()), np.argwhere(~same)[:4].tolist())


def test_tile_merge_batches_frames_and_takes_device_origins():
    from sleap_nn_amd.inference.tile_merger import build_importance_window, merge_tiles, origins_tensor

    ys, xs, t, F = [0, 10, 24], [0, 12, 20, 36], 16, 3
    tiles = torch.randn((F * len(ys) * len(xs), 5, t, t), generator=torch.Generator().manual_seed(3))
    win = build_importance_window((t, t))
    got = merge_tiles(tiles.to(DEV), win.to(DEV), origins_tensor(ys, DEV), origins_tensor(xs, DEV), (40, 52), frames=F)
    assert np.array_equal(_bits(got), _bits(_torch_merge(tiles, win, ys, xs, (40, 52), frames=F)))
    with pytest.raises(ValueError):
        merge_tiles(tiles.to(DEV), win, ys, xs, (40, 52), frames=2)
    with pytest.raises(ValueError):
        merge_tiles(tiles.to(DEV), win[:8], ys, xs, (40, 52), frames=F)


def test_tile_merge_uncovered_pixels_are_nan_where_the_torch_merger_has_them():
    from sleap_nn_amd.inference.tile_merger import build_importance_window, merge_tiles

    ys, xs, t = [0], [0, 40], 16  # rows 16.. and columns 16..39, 56.. are covered by no tile
    tiles = torch.rand((2, 3, t, t), generator=torch.Generator().manual_seed(4)) + 0.5
    win = build_importance_window((t, t), mode="pyramid")
    for hw in ((20, 60), (20, 59)):  # vector and scalar path
        got = merge_tiles(tiles.to(DEV), win, ys, xs, hw).cpu()
        want = _torch_merge(tiles, win, ys, xs, hw)
        assert torch.isnan(want).any() and not torch.isnan(want).all()
        assert torch.equal(torch.isnan(got), torch.isnan(want))
        assert np.array_equal(_bits(got)[~torch.isnan(want).numpy()], _bits(want)[~torch.isnan(want).numpy()])


# ---- TiledLayer ------------------------------------------------------------------------------------------------------------------
def _e2e_frames(image):
    """The twin of tools/gen_tiling_golden.py::e2e_frames: the end-to-end inputs by recipe name from the fixture frames."""
    fr = image[:, 0]
    return {"frame0": fr[:1], "batch2": fr[:2], "mosaic": np.tile(fr[:1], (1, 1, 2, 2)), "sub": fr[:1, :, 30:130, 100:220], "frame1": fr[1:2]}


@pytest.fixture(scope="module")
def assets():
    from sleap_nn_amd.inference.loaders import load_model_assets

    return load_model_assets(RUN_DIR)


@pytest.fixture(scope="module")
def backend(assets):
    from sleap_nn_amd.inference.backends import HipBackend

    return HipBackend(assets.build_model(), DEV)


@pytest.fixture(scope="module")
def frames():
    return _e2e_frames(G.load("ckpt_single_instance.npz")["image"])


def _inner(assets, backend, scale=1.0, peak_threshold=0.2, return_confmaps=True):
    from sleap_nn_amd.inference.layers import PostprocessConfig, PreprocessConfig, SingleInstanceLayer

    return SingleInstanceLayer(backend, assets.head_config["confmaps"]["output_stride"], max_stride=assets.backbone_config["max_stride"],
                               preprocess_config=PreprocessConfig(scale=scale), postprocess_config=PostprocessConfig(peak_threshold=peak_threshold, return_confmaps=return_confmaps))


def _check_against(out, want_cms, want_kp, want_vals, tag):
    cms, kp, vals = out.pred_confmaps.cpu().numpy(), out.pred_keypoints.cpu().numpy(), out.pred_peak_values.cpu().numpy()
    assert cms.shape == want_cms.shape and kp.shape == want_kp.shape and vals.shape == want_vals.shape, tag
    print(f"{tag}: confmaps max |d| {np.abs(cms - want_cms).max():.3e}, peak values {np.abs(vals - want_vals).max():.3e}, keypoints {np.nanmax(np.abs(kp - want_kp)):.3e} px")
    assert np.abs(cms - want_cms).max() <= CMS_ATOL, tag
    assert np.abs(vals - want_vals).max() <= CMS_ATOL, tag
    assert np.array_equal(np.isnan(kp), np.isnan(want_kp)), tag
    assert np.allclose(kp, want_kp, atol=KPT_ATOL, equal_nan=True), tag


def test_tiled_layer_reproduces_the_reference_run_on_every_recorded_case(z, assets, backend, frames):
    from sleap_nn_amd.inference.layers import TiledLayer

    cases = json.loads(str(z["e2e/cases"]))
    assert len(cases) >= 8 and {"frame0_t64", "frame0_t128", "mosaic_t128", "sub_t128"} <= set(cases)
    assert any(c[3] != 1.0 for c in cases.values()) and any(c[0] == "batch2" for c in cases.values())
    for name, (recipe, ts, ov, scale, blend) in cases.items():
        layer = TiledLayer(_inner(assets, backend, scale, float(z["e2e/peak_threshold"])), ts, ov, blend=blend)
        x = torch.from_numpy(frames[recipe])
        out = layer.predict(x)
        assert layer.tile_origins(tuple(z[f"e2e/{name}/processed_size"].tolist())) == [tuple(v) for v in z[f"e2e/{name}/origins"].tolist()], name
        info = out.preprocess_info
        assert tuple(info.processed_size) == tuple(z[f"e2e/{name}/processed_size"].tolist()) and tuple(info.original_size) == tuple(x.shape[-2:])
        assert info.input_scale == scale and info.output_stride == layer.output_stride
        assert out.pred_keypoints.shape == (x.shape[0], 1, 2, 2) and out.pred_peak_values.shape == (x.shape[0], 1, 2)
        _check_against(out, z[f"e2e/{name}/pred_confmaps"], z[f"e2e/{name}/pred_keypoints"], z[f"e2e/{name}/pred_peak_values"], name)


def test_tiled_layer_input_layouts_and_confmaps_off(assets, backend, frames):
    from sleap_nn_amd.inference.layers import TiledLayer

    layer = TiledLayer(_inner(assets, backend), 128, 32)
    ref = layer(torch.from_numpy(frames["frame0"]))
    hwc = layer.predict(np.ascontiguousarray(frames["frame0"][0].transpose(1, 2, 0)))  # (H, W, C) array
    assert torch.equal(hwc.pred_keypoints, ref.pred_keypoints) and torch.equal(hwc.pred_confmaps, ref.pred_confmaps)
    flt = layer.predict(torch.from_numpy(frames["frame0"]).float())  # float frames in 0..255: normalised per backend call, as in the reference
    assert torch.allclose(flt.pred_confmaps, ref.pred_confmaps, atol=1e-5)
    off = TiledLayer(_inner(assets, backend, return_confmaps=False), 128, 32).predict(torch.from_numpy(frames["frame0"]))
    assert off.pred_confmaps is None and torch.equal(off.pred_keypoints, ref.pred_keypoints)


def test_one_constant_tile_equals_the_plain_layer_on_the_padded_frame(assets, backend, frames):
    """One tile over the whole frame with ``blend="constant"`` is the plain layer on the frame padded to the tile: ``x * 1 / 1`` is exact.
    The stitched maps are the plain maps cropped to the frame, and the keypoints are the plain layer's wherever both search the same
    pixels.  The fixture model answers the edge of zero padding with a node-B response (0.56 - 0.68 in the first padded map row,
    on every sub-frame tried) above its true peak (0.33 - 0.51), so the plain layer's node B on a PADDED frame lies in the padding,
    which the tiled layer (like the reference's) crops away: the keypoints are therefore compared (a) with the plain layer itself on
    a frame of exactly the tile's size, (b) on the padded frame with the plain layer's maps searched over the frame's region."""
    from sleap_nn_amd.inference.layers import TiledLayer
    from sleap_nn_amd.inference.ops.peaks import find_global_peaks

    inner = _inner(assets, backend)
    tiled = TiledLayer(inner, 128, 32, blend="constant")
    # (a) no padding needed: the same maps, the same search region, the same keypoints
    x = torch.from_numpy(np.ascontiguousarray(frames["frame0"][:, :, 16:144, 76:204]))
    out, plain = tiled.predict(x), inner.predict(x)
    assert tiled.tile_origins((128, 128)) == [(0, 0)]
    assert np.abs(_bits(out.pred_confmaps).astype(np.int64) - _bits(plain.pred_confmaps).astype(np.int64)).max() <= 4
    assert not torch.isnan(out.pred_keypoints).any()
    assert torch.equal(torch.isnan(out.pred_keypoints), torch.isnan(plain.pred_keypoints))
    assert torch.allclose(out.pred_keypoints, plain.pred_keypoints, atol=KPT_ATOL, equal_nan=True)
    assert torch.equal(out.pred_peak_values, plain.pred_peak_values)
    # (b) 100 x 120, tile 128: one tile at (0, 0), zero padded
    x = torch.from_numpy(frames["sub"])
    out = tiled.predict(x)
    padded = torch.zeros((1, 3, 128, 128), dtype=torch.uint8)
    padded[:, :, :100, :120] = x
    plain = inner.predict(padded)
    a, b = _bits(out.pred_confmaps), _bits(plain.pred_confmaps[:, :, :25, :30])
    assert np.abs(a.astype(np.int64) - b.astype(np.int64)).max() <= 4  # in practice equal
    pk, pv = find_global_peaks(plain.pred_confmaps[:, :, :25, :30].contiguous(), threshold=0.2, refinement="integral", integral_patch_size=5)
    assert torch.equal(torch.isnan(out.pred_keypoints[:, 0]), torch.isnan(pk))
    assert torch.allclose(out.pred_keypoints[:, 0], pk * 4, atol=KPT_ATOL, equal_nan=True)
    assert torch.equal(out.pred_peak_values[:, 0], pv)


class _SpyBackend:
    def __init__(self, wrapped):
        self.wrapped = wrapped
        self.batch_sizes = []

    @property
    def device(self):
        return self.wrapped.device

    @property
    def does_baked_postproc(self):
        return False

    def __call__(self, x):
        assert x.dim() == 5 and x.shape[1] == 1  # (n, 1, C, ts, ts), as the reference hands tiles to its backend
        self.batch_sizes.append(int(x.shape[0]))
        return self.wrapped(x)

    def warmup(self, shape):
        self.wrapped.warmup(shape)


def test_tile_batch_size_bounds_every_backend_call(assets, backend, frames):
    from sleap_nn_amd.data import generate_tile_grid
    from sleap_nn_amd.inference.layers import TiledLayer

    assert len(generate_tile_grid((160, 280), 128, 64, 4, 4, 0.25)) == 8
    x = torch.from_numpy(frames["batch2"])
    outs = {}
    for tbs in (1, 3, 8):
        inner = _inner(assets, backend)
        spy = inner.backend = _SpyBackend(backend)
        outs[tbs] = TiledLayer(inner, 128, 64, tile_batch_size=tbs).predict(x)
        assert spy.batch_sizes and max(spy.batch_sizes) <= tbs and sum(spy.batch_sizes) == 16, (tbs, spy.batch_sizes)
        if tbs == 3:
            assert spy.batch_sizes == [3, 3, 3, 3, 3, 1]  # chunks run over the frame boundary
    for tbs in (1, 3):
        o, r = outs[tbs], outs[8]
        assert (o.pred_confmaps - r.pred_confmaps).abs().max().item() <= CMS_ATOL
        assert (o.pred_peak_values - r.pred_peak_values).abs().max().item() <= CMS_ATOL
        assert torch.allclose(o.pred_keypoints, r.pred_keypoints, atol=KPT_ATOL, equal_nan=True)


def test_graph_replay_gives_the_same_bits(assets, frames):
    """Same kernels with and without hipGraph replay; a replay that overwrote a chunk's maps before they were copied into the arena would show."""
    from sleap_nn_amd.inference.backends import HipBackend
    from sleap_nn_amd.inference.layers import TiledLayer

    x = torch.from_numpy(frames["batch2"])
    outs = []
    for use_graph in (False, True):
        be = HipBackend(assets.build_model(), DEV, use_graph=use_graph)
        layer = TiledLayer(_inner(assets, be), 128, 32, tile_batch_size=4)  # 12 tiles: three replays of one graph
        outs.append(layer.predict(x))
        if use_graph:
            outs.append(layer.predict(x))  # and once more from the captured graph alone
    for o in outs[1:]:
        assert np.array_equal(_bits(o.pred_confmaps), _bits(outs[0].pred_confmaps))
        assert torch.equal(o.pred_keypoints, outs[0].pred_keypoints) and torch.equal(o.pred_peak_values, outs[0].pred_peak_values)


@pytest.mark.parametrize("blend", BLENDS)
def test_host_accumulator_equals_the_device_stitch_bit_for_bit(assets, backend, frames, blend):
    from sleap_nn_amd.inference.layers import TiledLayer

    for recipe, ts, ov in (("batch2", 64, 16), ("sub", 128, 32), ("mosaic", 128, 96)):
        x = torch.from_numpy(frames[recipe])
        dev = TiledLayer(_inner(assets, backend), ts, ov, blend=blend, accumulator_device="cuda").predict(x)
        host = TiledLayer(_inner(assets, backend), ts, ov, blend=blend, accumulator_device="cpu").predict(x)
        auto = TiledLayer(_inner(assets, backend), ts, ov, blend=blend).predict(x)
        assert np.array_equal(_bits(dev.pred_confmaps), _bits(host.pred_confmaps)), (recipe, blend)
        assert np.array_equal(_bits(dev.pred_confmaps), _bits(auto.pred_confmaps))
        assert torch.equal(dev.pred_keypoints, host.pred_keypoints)


# ---- Predictor -------------------------------------------------------------------------------------------------------------------
def _run_dir_with_tiling(tmp_path, kind, tiling):
    dst = tmp_path / kind
    shutil.copytree(os.path.join(G.GOLDEN_DIR, "ckpt_dirs", kind), dst)
    cfg = yaml.safe_load(open(dst / "training_config.yaml"))
    cfg["data_config"]["preprocessing"]["tiling"] = tiling
    with open(dst / "training_config.yaml", "w") as f:
        yaml.safe_dump(cfg, f)
    return str(dst)


def test_predictor_routes_a_tiled_run_directory(tmp_path, frames):
    from sleap_nn_amd.inference.layers import SingleInstanceLayer, TiledLayer
    from sleap_nn_amd.inference.predictor import Predictor

    plain = Predictor.from_model_paths([RUN_DIR], device=DEV, batch_size=2)
    assert isinstance(plain.layer, SingleInstanceLayer) and len(plain.replicas) == 2  # untouched directory: exactly as before
    off = Predictor.from_model_paths([_run_dir_with_tiling(tmp_path / "off", "minimal_instance_single_instance", {"enabled": False, "tile_size": 64, "overlap": 16})], device=DEV)
    assert isinstance(off.layer, SingleInstanceLayer)

    d = _run_dir_with_tiling(tmp_path, "minimal_instance_single_instance", {"enabled": True, "tile_size": 64, "overlap": 16, "blend": "pyramid", "tile_batch_size": 4})
    pred = Predictor.from_model_paths([d], device=DEV, batch_size=2, return_confmaps=True, tile_size=64, overlap=16)
    layer = pred.layer
    assert isinstance(layer, TiledLayer) and isinstance(layer.inner, SingleInstanceLayer) and pred.replicas == []
    assert (layer.tile_size, layer.overlap, layer.tile_batch_size, layer._blend, layer.accumulator_device) == (64, 16, 4, "pyramid", "auto")
    assert layer.inner.preprocess_config.scale == 0.5  # the run directory's input scale applies; its sizematcher does not
    x = torch.from_numpy(np.concatenate([frames["batch2"], frames["batch2"][::-1]]))  # 4 frames: two batches
    outs = pred.predict(x)
    assert len(outs) == 2
    for i, o in enumerate(outs):
        direct = layer.predict(x[2 * i : 2 * i + 2])
        assert tuple(o.preprocess_info.processed_size) == (80, 140) and o.pred_confmaps.shape == (2, 2, 20, 35)
        assert o.frame_indices.tolist() == [2 * i, 2 * i + 1]
        assert torch.equal(o.pred_keypoints, direct.pred_keypoints) and torch.equal(o.pred_peak_values, direct.pred_peak_values)
        assert np.array_equal(_bits(o.pred_confmaps), _bits(direct.pred_confmaps))
    with pytest.raises(ValueError, match="tile_size override"):
        Predictor.from_model_paths([d], device=DEV, tile_size=128)
    with pytest.raises(ValueError, match="overlap override"):
        Predictor.from_model_paths([d], device=DEV, overlap=32)
    with pytest.raises(ValueError, match="tile_size"):
        Predictor.from_model_paths([_run_dir_with_tiling(tmp_path / "bad", "minimal_instance_single_instance", {"enabled": True, "overlap": 16})], device=DEV)


def test_predictor_refuses_tiling_for_other_model_types(tmp_path):
    from sleap_nn_amd.inference.predictor import Predictor

    d = _run_dir_with_tiling(tmp_path, "minimal_instance_bottomup", {"enabled": True, "tile_size": 128, "overlap": 32})
    with pytest.raises(NotImplementedError, match="bottomup"):
        Predictor.from_model_paths([d], device=DEV)
