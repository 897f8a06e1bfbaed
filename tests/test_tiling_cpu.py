"""Tiled inference, host side: the tile grid, the importance windows and the torch ``TileMerger`` against what the reference's
own functions produced (tests/golden/tiling.npz, written by tools/gen_tiling_golden.py), the properties the reference's tests
state, and the run-directory parsing.  No GPU."""
import json

import numpy as np
import pytest
import torch

from tests import _golden as G

BLENDS = ("gaussian", "pyramid", "constant")


@pytest.fixture(scope="module")
def z():
    return G.load("tiling.npz")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def test_tile_grid_equals_reference_over_the_sweep(z):
    from sleap_nn_amd.data import generate_tile_grid

    params, mof, flat, offs = z["grid/params"], z["grid/min_overlap_fraction"], z["grid/origins"], z["grid/offsets"]
    assert len(params) >= 25
    collapsed = repeated = below = False
    for i, (H, W, ts, ov, s, ms) in enumerate(params.tolist()):
        want = [tuple(v) for v in flat[offs[i] : offs[i + 1]].reshape(-1, 2).tolist()]
        got = generate_tile_grid((H, W), ts, ov, s, ms, float(mof[i]))
        assert got == want, (H, W, ts, ov, s, ms, mof[i])
        assert all(y % s == 0 and x % s == 0 for y, x in got)
        xs = sorted({x for _, x in got})
        collapsed |= len(xs) > 2 and xs[1] - xs[0] == s
        repeated |= W > ts and (W - ts) // s * s == 0  # the inward-snapped last origin is the walked origin 0 again: one tile, not two
        below |= H < ts and W < ts and got == [(0, 0)]
    assert collapsed and repeated and below  # the sweep holds the corner cases it is meant to hold
    # defaults of the signature: max_stride 1, min_overlap_fraction 0.25
    assert generate_tile_grid((160, 280), 128, 32, 4) == generate_tile_grid((160, 280), 128, 32, 4, 1, 0.25)


def test_importance_windows_equal_reference(z):
    from sleap_nn_amd.inference.tile_merger import build_importance_window

    for th, tw in z["window/sizes"].tolist():
        for mode in BLENDS:
            got = build_importance_window((th, tw), mode=mode)
            want = z[f"window/{mode}/{th}x{tw}"]
            assert got.dtype == torch.float32 and tuple(got.shape) == (th, tw)
            if mode == "gaussian":  # torch.exp may differ in the last place between host CPUs; nothing else in the expression can
                assert np.abs(_bits(got.numpy()).astype(np.int64) - _bits(want).astype(np.int64)).max() <= 2, (mode, th, tw)
            else:
                assert np.array_equal(_bits(got.numpy()), _bits(want)), (mode, th, tw)
            assert float(got.min()) >= 1e-3 and float(got.max()) <= 1.0
    got = build_importance_window((16, 12), mode="gaussian", sigma_scale=0.25).numpy()
    assert np.abs(_bits(got).astype(np.int64) - _bits(z["window/gaussian_s0.25/16x12"]).astype(np.int64)).max() <= 2
    assert build_importance_window((4, 4), dtype=torch.float64).dtype == torch.float64


def test_unknown_blend_raises():
    from sleap_nn_amd.inference.tile_merger import build_importance_window

    with pytest.raises(ValueError, match="Unknown importance window mode"):
        build_importance_window((8, 8), mode="hann")


def test_torch_merger_equals_reference_bit_for_bit(z):
    """Elementwise float32 mul / add / div: identical on every IEEE host, so ``view(int32)`` equality, signed zeros and denormals included."""
    from sleap_nn_amd.inference.tile_merger import TileMerger

    names = json.loads(str(z["merge/names"]))
    assert len(names) >= 5
    for name in names:
        tiles = torch.from_numpy(z[f"merge/{name}/tiles"])
        ys, xs = z[f"merge/{name}/y_origins"].tolist(), z[f"merge/{name}/x_origins"].tolist()
        h, w = z[f"merge/{name}/out_hw"].tolist()
        t = tiles.shape[-1]
        for mode in BLENDS:
            m = TileMerger((max(h, t), max(w, t)), tiles.shape[1], torch.from_numpy(z[f"merge/{name}/{mode}/window"]))
            for k, (y0, x0) in enumerate((y0, x0) for y0 in ys for x0 in xs):
                m.integrate(tiles[k], y0, x0)
            got = m.merge()[:, :h, :w].numpy()
            assert np.array_equal(_bits(got), _bits(z[f"merge/{name}/{mode}/merged"])), (name, mode)


def test_torch_merger_clipped_partial_tiles(z):
    from sleap_nn_amd.inference.tile_merger import TileMerger

    tiles = torch.from_numpy(z["merge/partial/tiles"])
    h, w = z["merge/partial/out_hw"].tolist()
    m = TileMerger((h, w), tiles.shape[1], torch.from_numpy(z["merge/partial/window"]))
    for k, (y0, x0) in enumerate(z["merge/partial/places"].tolist()):
        m.integrate(tiles[k][:, : h - y0, : w - x0], y0, x0)
    assert np.array_equal(_bits(m.merge().numpy()), _bits(z["merge/partial/merged"]))
    assert np.array_equal(_bits(m.merge(eps=1e-6).numpy()), _bits(z["merge/partial/merged_eps"]))


@pytest.mark.parametrize("mode", BLENDS)
def test_merger_uniform_field_reconstruction(mode):
    """A uniform field stitches back to itself wherever it is covered, whatever the window (sum-of-weights normalisation)."""
    from sleap_nn_amd.data import generate_tile_grid
    from sleap_nn_amd.inference.tile_merger import TileMerger, build_importance_window

    H, W, t = 40, 56, 16
    win = build_importance_window((t, t), mode=mode)
    m = TileMerger((H, W), 3, win)
    for y0, x0 in generate_tile_grid((H, W), t, 4, 1):
        m.integrate(torch.full((3, t, t), 0.7), y0, x0)
    out = m.merge()
    assert not torch.isnan(out).any()
    assert torch.allclose(out, torch.full_like(out, 0.7), atol=1e-6)


def test_merger_weighted_average_of_two_values_and_uncovered_nan():
    from sleap_nn_amd.inference.tile_merger import TileMerger

    win = torch.tensor([[1.0, 0.25]])
    m = TileMerger((1, 4), 1, win)
    m.integrate(torch.full((1, 1, 2), 2.0), 0, 0)  # weights 1, 0.25 at x = 0, 1
    m.integrate(torch.full((1, 1, 2), 6.0), 0, 1)  # weights 1, 0.25 at x = 1, 2
    out = m.merge()[0, 0]
    assert out[0] == 2.0 and out[2] == 6.0
    assert out[1] == pytest.approx((0.25 * 2.0 + 1.0 * 6.0) / 1.25)
    assert torch.isnan(out[3])  # never covered
    assert m.merge(eps=1e-6)[0, 0, 3] == 0.0


def test_merger_accumulates_fp16_tiles_in_float32():
    from sleap_nn_amd.inference.tile_merger import TileMerger

    m = TileMerger((4, 4), 2, torch.ones((4, 4)))
    tile = torch.full((2, 4, 4), 1.0 + 2.0**-10, dtype=torch.float16)
    for _ in range(3):
        m.integrate(tile, 0, 0)
    assert m.acc.dtype == torch.float32 and m.cnt.dtype == torch.float32
    assert m.merge().dtype == torch.float32
    assert torch.equal(m.acc, torch.full((2, 4, 4), 3.0 * (1.0 + 2.0**-10)))  # exact in float32, not representable in float16


def test_tiling_block_is_parsed_with_defaults():
    from sleap_nn_amd.inference.layers.tiled import tiling_kwargs

    assert tiling_kwargs({}) is None and tiling_kwargs(None) is None
    assert tiling_kwargs({"scale": 0.5, "tiling": None}) is None
    assert tiling_kwargs({"tiling": {"enabled": False, "tile_size": 128, "overlap": 32}}) is None
    kw = tiling_kwargs({"tiling": {"enabled": True, "tile_size": 128, "overlap": 32}})
    assert kw == {"tile_size": 128, "overlap": 32, "min_overlap_fraction": 0.25, "blend": "gaussian", "sigma_scale": 0.125, "tile_batch_size": 8,
                  "accumulator_device": "auto", "cpu_thresh": 0.40}
    kw = tiling_kwargs({"tiling": {"enabled": True, "tile_size": 256, "overlap": 64, "blend": "pyramid", "tile_batch_size": 3, "accumulator_device": "cpu",
                                   "sigma_scale": 0.2, "min_overlap_fraction": 0.3, "cpu_thresh": 0.1, "sampling": "grid", "tile_batch_size_hint": None}})
    assert kw == {"tile_size": 256, "overlap": 64, "min_overlap_fraction": 0.3, "blend": "pyramid", "sigma_scale": 0.2, "tile_batch_size": 3,
                  "accumulator_device": "cpu", "cpu_thresh": 0.1}
    assert tiling_kwargs({"tiling": {"enabled": True, "tile_size": 128, "overlap": 32, "tile_batch_size": None}})["tile_batch_size"] == 8


def test_enabled_tiling_without_geometry_raises():
    from sleap_nn_amd.inference.layers.tiled import tiling_kwargs

    with pytest.raises(ValueError, match="tile_size"):
        tiling_kwargs({"tiling": {"enabled": True, "overlap": 32}})
    with pytest.raises(ValueError, match="tile_size"):
        tiling_kwargs({"tiling": {"enabled": True, "tile_size": None, "overlap": 32}})
    with pytest.raises(ValueError, match="overlap"):
        tiling_kwargs({"tiling": {"enabled": True, "tile_size": 128, "overlap": "32"}})


def test_tiling_override_is_checked_not_applied():
    from sleap_nn_amd.inference.layers.tiled import tiling_kwargs

    pre = {"tiling": {"enabled": True, "tile_size": 128, "overlap": 32}}
    assert tiling_kwargs(pre, tile_size=128, overlap=32)["tile_size"] == 128
    with pytest.raises(ValueError, match="tile_size override"):
        tiling_kwargs(pre, tile_size=256)
    with pytest.raises(ValueError, match="overlap override"):
        tiling_kwargs(pre, overlap=16)
    assert tiling_kwargs({"tiling": {"enabled": False}}, tile_size=256) is None  # no-op unless tiling is enabled


def test_tiled_layer_validates_its_arguments():
    from sleap_nn_amd.inference.layers import TiledLayer

    class _Backend:
        device = "cpu"
        does_baked_postproc = False

    class _Inner:
        backend = _Backend()
        output_stride = 4
        max_stride = 16

    assert TiledLayer(_Inner(), 128, 32).tile_origins((160, 280)) == [(0, 0), (0, 96), (0, 152), (32, 0), (32, 96), (32, 152)]
    for bad in (0, -16, 100, 120):  # not positive / not a multiple of max_stride 16
        with pytest.raises(ValueError, match="tile_size"):
            TiledLayer(_Inner(), bad, 32)
    with pytest.raises(ValueError, match="Unknown importance window mode"):
        TiledLayer(_Inner(), 128, 32, blend="hann")
    with pytest.raises(ValueError, match="accumulator_device"):
        TiledLayer(_Inner(), 128, 32, accumulator_device="tpu")

    class _Baked(_Inner):
        class backend:
            device = "cpu"
            does_baked_postproc = True

    with pytest.raises(NotImplementedError):
        TiledLayer(_Baked(), 128, 32)


def test_loader_exposes_the_tiling_block(tmp_path):
    """``load_model_assets`` hands ``data_config.preprocessing`` through, tiling block included (what ``_select_layer`` reads)."""
    import os
    import shutil

    import yaml

    from sleap_nn_amd.inference.layers.tiled import tiling_kwargs
    from sleap_nn_amd.inference.loaders import load_model_assets

    src = os.path.join(G.GOLDEN_DIR, "ckpt_dirs", "minimal_instance_single_instance")
    assert tiling_kwargs(load_model_assets(src).preprocessing) is None
    dst = tmp_path / "tiled_run"
    shutil.copytree(src, dst)
    cfg = yaml.safe_load(open(dst / "training_config.yaml"))
    cfg["data_config"]["preprocessing"]["tiling"] = {"enabled": True, "tile_size": 128, "overlap": 32, "blend": "pyramid"}
    yaml.safe_dump(cfg, open(dst / "training_config.yaml", "w"))
    kw = tiling_kwargs(load_model_assets(str(dst)).preprocessing)
    assert (kw["tile_size"], kw["overlap"], kw["blend"], kw["tile_batch_size"]) == (128, 32, "pyramid", 8)
