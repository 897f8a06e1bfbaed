"""Generate tests/golden/tiling.npz from the reference's own tiled-inference code.

Runs, through ``oracle.ref_harness`` (where the reference tree is available):

1. ``sleap_nn.data.tiling.generate_tile_grid`` over a parameter sweep (frames below / equal to / above the tile, sizes that are
   not multiples of the stride, overlaps below and above the ``min_overlap_fraction`` floor, ``max_stride`` compatible and
   incompatible with ``output_stride``, a step that collapses to ``output_stride``, a last origin that repeats the previous one);
2. ``sleap_nn.inference.tile_merger.build_importance_window`` for the three modes on square / non-square, odd / even sizes;
3. ``TileMerger`` on seeded random tile maps (negative values, exact zeros, a denormal-scale channel) with 1, 2 and 3-or-more
   tiles covering a pixel per axis, for each blend, plus one case of clipped partial tiles;
4. the reference's ``TiledLayer`` on ``TorchBackend(cpu)`` around the ``minimal_instance_single_instance`` fixture checkpoint
   (tests/golden/ckpt_dirs/) on frames built from the fixture frames of tests/golden/ckpt_single_instance.npz by the recipes
   of ``e2e_frames`` below (tests rebuild them the same way: only the recipe's name is stored).

For every recorded stitched map the generator asserts that each node's maximum exceeds the largest value outside its 5 x 5
patch by at least 1e-3, and lies at least 1e-3 from ``peak_threshold``: ten times the 1e-4 tolerance the maps are compared
with, so neither the argmax nor the NaN mask can flip.  A case that misses the margin is dropped (and reported); the required
kinds of case must survive.

The reference's ``resize_image`` calls torchvision (absent here, stubbed by the harness): as in
``oracle/gen_golden.py::topdown_sized_fixture`` that one call is replaced by the torch operator it dispatches to,
``F.interpolate(mode="bilinear", antialias=True)``.

    python tools/gen_tiling_golden.py [out.npz]
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np
import torch
import yaml

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MARGIN = 1e-3
PEAK_THRESHOLD = 0.2
BLENDS = ("gaussian", "pyramid", "constant")

# (H, W, tile_size, overlap, output_stride, max_stride, min_overlap_fraction)
GRID_SWEEP = [
    (160, 280, 128, 32, 4, 4, 0.25), (160, 280, 64, 16, 4, 4, 0.25), (160, 280, 128, 64, 4, 4, 0.25), (320, 560, 128, 32, 4, 4, 0.25),
    (100, 120, 128, 32, 4, 4, 0.25),  # frame below the tile on both axes
    (128, 128, 128, 32, 4, 4, 0.25),  # equal to the tile
    (128, 300, 128, 32, 4, 16, 0.25),  # one axis equal, one above
    (130, 257, 128, 32, 4, 4, 0.25),  # barely above: the last origin lands on the stride grid below dim - tile
    (161, 283, 64, 16, 4, 4, 0.25), (203, 517, 96, 8, 2, 16, 0.25),  # non-multiples of the stride
    (512, 512, 128, 0, 4, 16, 0.25), (512, 512, 128, 8, 4, 16, 0.25),  # overlap below the floor: raised to 32
    (512, 512, 128, 96, 4, 16, 0.25), (512, 512, 128, 48, 4, 16, 0.0),  # above the floor / no floor
    (512, 512, 128, 32, 4, 6, 0.25), (512, 512, 128, 32, 8, 12, 0.25),  # max_stride incompatible with output_stride
    (512, 512, 128, 32, 2, 32, 0.25), (640, 384, 256, 64, 2, 32, 0.25),  # compatible
    (300, 300, 128, 120, 4, 16, 0.25),  # step 8 < max_stride: snaps to output_stride
    (200, 200, 128, 127, 4, 4, 0.25), (150, 140, 128, 128, 8, 8, 0.25), (96, 200, 64, 70, 4, 4, 0.25),  # step collapses to output_stride
    (192, 256, 128, 64, 4, 4, 0.25), (384, 384, 128, 0, 4, 4, 0.5),  # walked origins stop right at dim - tile
    (132, 260, 128, 124, 4, 4, 0.25),  # (132 - 128 = 4: one walked origin, the last origin 4)
    (131, 129, 128, 32, 4, 4, 0.25),  # last origin (dim - tile) // stride * stride = 0 repeats the walked origin 0
    (4096, 4096, 512, 128, 2, 16, 0.25), (1024, 1280, 256, 64, 4, 32, 0.25),
]

WINDOW_SIZES = [(8, 8), (7, 7), (16, 12), (9, 14), (32, 32), (1, 5), (33, 16)]

# name -> (tile th = tw, y origins, x origins, canvas (h, w)); origins and sizes in output-stride pixels
MERGE_CASES = {
    "one_tile": (16, [0], [0], (16, 16)),
    "one_tile_cropped": (16, [0], [0], (10, 13)),  # frame below the tile: the canvas is the tile, the result is cropped
    "two_per_axis": (16, [0, 12], [0, 8, 20], (28, 36)),
    "three_per_axis": (16, [0, 4, 8, 12, 16], [0, 6, 12, 18, 20], (32, 36)),
    "dense_step1": (8, [0, 1, 2, 3], [0, 1, 2, 3, 4, 5], (11, 13)),  # the step collapsed to the stride: up to 4 x 6 tiles on a pixel
    "unaligned_x": (12, [0, 7], [0, 5, 9, 14], (19, 26)),  # origins that are not multiples of 4
}


def grids(ref_grid):
    table, flat, offs = [], [], [0]
    for (H, W, ts, ov, s, ms, mof) in GRID_SWEEP:
        g = ref_grid((H, W), ts, ov, s, ms, mof)
        table.append([H, W, ts, ov, s, ms])
        flat += [v for yx in g for v in yx]
        offs.append(len(flat))
    return {"grid/params": np.array(table, dtype=np.int64), "grid/min_overlap_fraction": np.array([p[6] for p in GRID_SWEEP], dtype=np.float64),
            "grid/origins": np.array(flat, dtype=np.int64), "grid/offsets": np.array(offs, dtype=np.int64)}


def windows(ref_window):
    out = {"window/sizes": np.array(WINDOW_SIZES, dtype=np.int64)}
    for mode in BLENDS:
        for (th, tw) in WINDOW_SIZES:
            out[f"window/{mode}/{th}x{tw}"] = ref_window((th, tw), mode=mode).numpy()
    out["window/gaussian_s0.25/16x12"] = ref_window((16, 12), mode="gaussian", sigma_scale=0.25).numpy()
    return out


def merge_tile_maps(name: str, n_tiles: int, t: int) -> torch.Tensor:
    """(n_tiles, 4, t, t): channel 0 N(0, 1), channel 1 uniform [0, 1) with a quarter of exact zeros, channel 2 at denormal scale
    (1e-41 .. 1e-38), channel 3 negative with signed zeros."""
    g = torch.Generator().manual_seed(1000 + sum(name.encode()))
    a = torch.randn((n_tiles, t, t), generator=g)
    b = torch.rand((n_tiles, t, t), generator=g)
    b[torch.rand((n_tiles, t, t), generator=g) < 0.25] = 0.0
    c = (torch.rand((n_tiles, t, t), generator=g).double() * 1e-38 + 1e-41).float() * torch.where(torch.rand((n_tiles, t, t), generator=g) < 0.5, -1.0, 1.0)
    d = -torch.rand((n_tiles, t, t), generator=g)
    d[torch.rand((n_tiles, t, t), generator=g) < 0.2] = -0.0
    return torch.stack([a, b, c, d], dim=1).contiguous()


def merges(ref_window, RefMerger):
    out = {"merge/names": np.array(json.dumps(list(MERGE_CASES)))}
    for name, (t, ys, xs, (h, w)) in MERGE_CASES.items():
        tiles = merge_tile_maps(name, len(ys) * len(xs), t)
        out[f"merge/{name}/tiles"] = tiles.numpy()
        out[f"merge/{name}/y_origins"], out[f"merge/{name}/x_origins"] = np.array(ys, dtype=np.int32), np.array(xs, dtype=np.int32)
        out[f"merge/{name}/out_hw"] = np.array([h, w], dtype=np.int64)
        for mode in BLENDS:
            win = ref_window((t, t), mode=mode)
            m = RefMerger((max(h, t), max(w, t)), tiles.shape[1], win)  # the canvas of tiled.py:236-237, cropped as :263
            for k, (y0, x0) in enumerate((y0, x0) for y0 in ys for x0 in xs):
                m.integrate(tiles[k], y0, x0)
            out[f"merge/{name}/{mode}/window"] = win.numpy()
            out[f"merge/{name}/{mode}/merged"] = m.merge()[:, :h, :w].numpy()
    # clipped partial tiles through integrate (the torch class only): tiles cut at the canvas's bottom / right edge
    t, (h, w) = 16, (24, 27)
    tiles = merge_tile_maps("partial", 4, t)
    win = ref_window((t, t), mode="gaussian")
    m = RefMerger((h, w), 4, win)
    places = [(0, 0), (0, 12), (12, 0), (12, 12)]
    for k, (y0, x0) in enumerate(places):
        m.integrate(tiles[k][:, : h - y0, : w - x0], y0, x0)
    out.update({"merge/partial/tiles": tiles.numpy(), "merge/partial/places": np.array(places, dtype=np.int64), "merge/partial/out_hw": np.array([h, w]),
                "merge/partial/window": win.numpy(), "merge/partial/merged": m.merge().numpy(), "merge/partial/merged_eps": m.merge(eps=1e-6).numpy()})
    return out


def e2e_frames(image: np.ndarray) -> dict:
    """The end-to-end inputs by name, from the fixture frames ``image (2, 1, 3, 160, 280)`` uint8.  tests/test_gpu_tiling.py imports this
    table's twin (``tests/test_gpu_tiling.py::_e2e_frames``); keep them in step."""
    fr = image[:, 0]  # (2, 3, 160, 280)
    return {"frame0": fr[:1], "batch2": fr[:2], "mosaic": np.tile(fr[:1], (1, 1, 2, 2)), "sub": fr[:1, :, 30:130, 100:220], "frame1": fr[1:2]}


# name -> (frames recipe, tile_size, overlap, input scale, blend)
E2E_CASES = {
    "frame0_t64": ("frame0", 64, 16, 1.0, "gaussian"),
    "frame0_t128": ("frame0", 128, 32, 1.0, "gaussian"),
    "frame1_t128_pyramid": ("frame1", 128, 32, 1.0, "pyramid"),
    "frame0_t64_constant": ("frame0", 64, 16, 1.0, "constant"),
    "mosaic_t128": ("mosaic", 128, 32, 1.0, "gaussian"),
    "sub_t128": ("sub", 128, 32, 1.0, "gaussian"),  # 100 x 120: smaller than the tile
    "mosaic_scale0.5_t64": ("mosaic", 64, 16, 0.5, "gaussian"),
    "mosaic_scale0.5_t128": ("mosaic", 128, 32, 0.5, "gaussian"),
    "batch2_t128": ("batch2", 128, 32, 1.0, "gaussian"),
    "batch2_t64": ("batch2", 64, 16, 1.0, "gaussian"),
}
E2E_REQUIRED = [("frame0_t64",), ("frame0_t128",), ("mosaic_t128",), ("sub_t128",), ("mosaic_scale0.5_t64", "mosaic_scale0.5_t128"), ("batch2_t128", "batch2_t64")]


def margins(cms: np.ndarray, vals: np.ndarray) -> float:
    """Smallest, over frames and nodes, of: maximum minus the largest value outside its 5 x 5 patch; |maximum - peak_threshold|."""
    worst = np.inf
    for b in range(cms.shape[0]):
        for n in range(cms.shape[1]):
            m = cms[b, n]
            y, x = np.unravel_index(np.argmax(m), m.shape)
            outside = m.copy()
            outside[max(0, y - 2) : y + 3, max(0, x - 2) : x + 3] = -np.inf
            worst = min(worst, float(m[y, x] - outside.max()), abs(float(m[y, x]) - PEAK_THRESHOLD))
            assert abs(float(vals[b, 0, n]) - float(m[y, x])) < 1e-6 or np.isnan(vals[b, 0, n])
    return worst


def end_to_end():
    import torch.nn as nn
    import torch.nn.functional as F

    import sleap_nn.data.resizing as rresizing
    from oracle import ref_harness as rh
    from sleap_nn.architectures.model import Model
    from sleap_nn.inference.layers.backends.torch_backend import TorchBackend
    from sleap_nn.inference.layers.configs import PostprocessConfig, PreprocessConfig
    from sleap_nn.inference.layers.single_instance import SingleInstanceLayer
    from sleap_nn.inference.layers.tiled import TiledLayer

    def tv_resize(image, size, **_kw):  # the torch operator torchvision's tensor resize dispatches to
        x = image if image.dim() == 4 else image[None]
        y = F.interpolate(x if x.dtype == torch.uint8 else x.float(), size=tuple(size), mode="bilinear", align_corners=False, antialias=True)
        return y if image.dim() == 4 else y[0]

    rresizing.tvf.resize = tv_resize

    class Fwd(nn.Module):  # the LightningModule forward preamble: squeeze the n_samples axis, normalize
        def __init__(self, m):
            super().__init__()
            self.m = m

        def forward(self, x):
            x = torch.squeeze(x, dim=1)
            if x.dtype == torch.uint8 or x.max() > 1.0:
                x = x.float() / 255.0
            return self.m(x.float())

    d = os.path.join(ROOT, "tests", "golden", "ckpt_dirs", "minimal_instance_single_instance")
    cfg = yaml.safe_load(open(os.path.join(d, "training_config.yaml")))
    bb = cfg["model_config"]["backbone_config"]["unet"]
    heads = cfg["model_config"]["head_configs"]["single_instance"]
    model = Model("unet", rh.attrdict(bb), rh.attrdict(heads), "single_instance").eval()
    model.load_state_dict(rh.load_lightning_ckpt_state(os.path.join(d, "best.ckpt")), strict=True)
    stride = heads["confmaps"]["output_stride"]
    frames = e2e_frames(np.load(os.path.join(ROOT, "tests", "golden", "ckpt_single_instance.npz"))["image"])

    out, kept = {}, []
    for name, (recipe, ts, ov, scale, blend) in E2E_CASES.items():
        inner = SingleInstanceLayer(TorchBackend(Fwd(model), device="cpu"), stride, max_stride=bb["max_stride"], preprocess_config=PreprocessConfig(scale=scale),
                                    postprocess_config=PostprocessConfig(peak_threshold=PEAK_THRESHOLD, return_confmaps=True))
        layer = TiledLayer(inner, tile_size=ts, overlap=ov, blend=blend, accumulator_device="cpu")
        with torch.inference_mode():
            o = layer.predict(torch.from_numpy(frames[recipe]))
        cms, kp, vals = o.pred_confmaps.numpy(), o.pred_keypoints.numpy(), o.pred_peak_values.numpy()
        proc = tuple(int(v) for v in o.preprocess_info.processed_size)
        from sleap_nn.data.tiling import generate_tile_grid

        origins = generate_tile_grid(proc, ts, ov, stride, bb["max_stride"], 0.25)
        mg = margins(cms, vals)
        ok = mg >= MARGIN
        print(f"e2e[{name}]: frames {frames[recipe].shape} -> processed {proc}, {len(origins)} tiles, peak values {np.round(vals.reshape(-1), 3).tolist()}, "
              f"margin {mg:.2e} {'kept' if ok else 'DROPPED (below 1e-3)'}")
        if not ok:
            continue
        kept.append(name)
        out.update({f"e2e/{name}/pred_keypoints": kp, f"e2e/{name}/pred_peak_values": vals, f"e2e/{name}/pred_confmaps": cms,
                    f"e2e/{name}/origins": np.array(origins, dtype=np.int64), f"e2e/{name}/processed_size": np.array(proc, dtype=np.int64)})
    for group in E2E_REQUIRED:
        assert any(n in kept for n in group), f"no end-to-end case of {group} met the {MARGIN} argmax / threshold margin"
    out["e2e/cases"] = np.array(json.dumps({n: list(E2E_CASES[n]) for n in kept}))
    out["e2e/peak_threshold"] = np.array(PEAK_THRESHOLD)
    return out


def main(path: str) -> None:
    from oracle import ref_harness as rh

    rh.install()
    from sleap_nn.data.tiling import generate_tile_grid
    from sleap_nn.inference.tile_merger import TileMerger, build_importance_window

    torch.set_num_threads(4)
    arrs = {}
    arrs.update(grids(generate_tile_grid))
    arrs.update(windows(build_importance_window))
    arrs.update(merges(build_importance_window, TileMerger))
    arrs.update(end_to_end())
    np.savez_compressed(path, **arrs)
    print(f"wrote {path} ({os.path.getsize(path) / 1024:.0f} KiB, {len(arrs)} arrays)")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "tiling.npz"))
