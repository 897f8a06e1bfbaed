"""Generate the tiled-segmentation goldens from the reference's own code (through ``oracle.ref_harness``, where the reference tree is available):

* ``tests/golden/tiled_segmentation.npz``
  - ``bu/<case>/...``: the reference's ``TiledSegmentationLayer`` over ``TorchBackend(cpu)`` with the committed ``tiny_bottomup_segmentation`` weights.
    Cases ``t64`` (two 90 x 134 frames, tile 64, overlap 16, gaussian, ``tile_batch_size`` 5), ``t32`` (tile 32, overlap 16, pyramid) and ``tiny`` (one
    40 x 56 frame, smaller than the 64-pixel tile).  Recorded: the frames and parameters, every tile's head maps in grid order (``tiles``: (F * T, 4, th, tw),
    channels foreground / centre / offset x / offset y), the stitched 4-channel map per frame as ``inner.postprocess`` received it, the ``pred_masks`` entries
    and the uncertain set;
  - ``sem/<case>/...``: the reference's ``TiledSemanticSegmentationLayer``, cases ``t64`` / ``t32`` on the same frames, one head.  Its tile maps and stitched map
    are channel 0 of the ``bu/<case>`` arrays bit for bit (asserted at generation), so frames / tiles / stitched are read from there and only the entries, the
    uncertain set and the parameters are stored;
  - ``merger/<case>/...``: seeded random 4-channel tiles through the reference's ``TileMerger``: ``odd`` (45 x 67 canvas) and ``vec`` (44 x 68 canvas,
    ``w % 4 == 0`` with x origins that are no multiples of 4).
* ``tests/golden/ckpt_dirs/tiny_tiled_semantic_segmentation``: the bottom-up checkpoint's backbone and its ``SegmentationHead`` (whose foreground is tuned) as a
  ``semantic_segmentation`` run directory.  The committed weights of ``tiny_bottomup_segmentation`` are read, never written.

Margins are those of ``gen_segmentation_golden.py::run_dir_case``, applied to the STITCHED maps: peak values at least 1e-3 from the threshold and from each
other, the NMS candidate structure clear by 1e-3, no plateau; uncertain set = foreground within 1e-3 of ``fg_threshold``, or the two nearest centres within
1e-3 relative; at most 0.5 % of a frame's pixels, and at least 2 instances per frame for ``t64`` / ``t32``.  The search is over FRAME seeds
(the first of 300 that qualifies: about one in eight for tile 64, about one in sixty for tile 32, where twenty-odd centres per frame leave many pixels near a tie).

    python tools/gen_tiled_seg_golden.py
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_segmentation_golden as gs  # noqa: E402

GOLD = gs.GOLD
MARGIN = gs.MARGIN
P = dict(fg_threshold=0.5, peak_threshold=0.2, output_stride=2, center_nms_kernel=3)
SEEDS = 300  # frame seeds tried per case (the first that meets every margin is recorded)
KEYS = ("SegmentationHead", "InstanceCenterHead", "CenterOffsetHead")
BU_CASES = {  # name -> frames (F, H, W), tile, overlap, blend, tile_batch_size, minimum instances per frame
    "t64": dict(F=2, H=90, W=134, tile_size=64, overlap=16, blend="gaussian", tile_batch_size=5, min_inst=2),
    "t32": dict(F=2, H=90, W=134, tile_size=32, overlap=16, blend="pyramid", tile_batch_size=8, min_inst=2),
    "tiny": dict(F=1, H=40, W=56, tile_size=64, overlap=16, blend="gaussian", tile_batch_size=8, min_inst=0),
}


def frames_for(seed, F, H, W):
    """``F`` uint8 frames of H x W: a few bright disks on a dim textured background (after ``run_dir_frames``, which keeps its disks' centres 12 pixels off every edge).  THIS
    generator keeps them 12 pixels off the left, top and right edges and ``min(30, H // 2)`` pixels off the bottom edge: its own choice, made because with 12 pixels
    all round no seed of 300 met the margins for tile 32."""
    g = np.random.default_rng(seed)
    fr = np.zeros((F, 1, H, W), dtype=np.float64)
    yy, xx = np.mgrid[0:H, 0:W]
    for b in range(F):
        fr[b, 0] = 30 + 10 * g.standard_normal((H, W))
        for _ in range(4):
            cx, cy, r = g.uniform(12, W - 12), g.uniform(12, max(H - 30, H // 2)), g.uniform(6, 11)
            fr[b, 0][(xx - cx) ** 2 + (yy - cy) ** 2 <= r * r] = g.uniform(150, 240)
    return np.clip(fr, 0, 255).astype(np.uint8)


def load_models(rh):
    """The committed bottom-up weights in the reference's ``Model``, and a semantic ``Model`` holding their backbone and ``SegmentationHead``."""
    sd = torch.load(os.path.join(GOLD, "ckpt_dirs", "tiny_bottomup_segmentation", "best.ckpt"), map_location="cpu", weights_only=False)["state_dict"]
    sd = {k[len("model."):]: v for k, v in sd.items()}
    bu = gs.seeded_model(rh, "bottomup_segmentation", 0)
    bu.load_state_dict(sd, strict=True)
    sem = gs.seeded_model(rh, "semantic_segmentation", 0)
    want = list(sem.state_dict().keys())
    missing = [k for k in want if k not in sd]
    assert not missing, f"the bottom-up key layout does not carry over: {missing}"
    sem.load_state_dict({k: sd[k] for k in want}, strict=True)
    return bu.eval(), sem.eval()


def make_fwd(m):
    import torch.nn as nn

    class Fwd(nn.Module):
        def __init__(self, m):
            super().__init__()
            self.m = m

        def forward(self, x):
            x = torch.squeeze(x, dim=1)
            if x.dtype == torch.uint8 or x.max() > 1.0:
                x = x.float() / 255.0
            out = self.m(x.float())
            return {k: (torch.sigmoid(v) if k == "SegmentationHead" else v) for k, v in out.items()}

    return Fwd(m)


def run_reference(model, frames, case, semantic):
    """The reference's tiled layer on ``frames``: (tile maps (F * T, C, th, tw) in grid order, stitched (F, C, h, w), pred_masks)."""
    from sleap_nn.inference.layers.backends.torch_backend import TorchBackend
    from sleap_nn.inference.layers.configs import PostprocessConfig, PreprocessConfig
    from sleap_nn.inference.layers.segmentation import SegmentationLayer, SemanticSegmentationLayer
    from sleap_nn.inference.layers.tiled import TiledSegmentationLayer, TiledSemanticSegmentationLayer

    backend = TorchBackend(make_fwd(model), device="cpu")
    kw = dict(max_stride=gs.BB["max_stride"], preprocess_config=PreprocessConfig(ensure_grayscale=True), postprocess_config=PostprocessConfig(peak_threshold=P["peak_threshold"]))
    inner = (SemanticSegmentationLayer if semantic else SegmentationLayer)(backend, 2, **kw)
    keys = KEYS[:1] if semantic else KEYS
    tile_maps, stitched = [], []

    class Recording:
        device = backend.device
        does_baked_postproc = getattr(backend, "does_baked_postproc", False)

        def __call__(self, x):
            raw = backend(x)
            tile_maps.append(torch.cat([raw[k] for k in keys], dim=1).detach().clone())
            return raw

        def __getattr__(self, name):
            return getattr(backend, name)

    inner.backend = Recording()
    post = inner.postprocess

    def spy(raw_out, info):
        stitched.append(torch.cat([raw_out[k] for k in keys], dim=1).detach().clone())
        return post(raw_out, info)

    inner.postprocess = spy
    layer = (TiledSemanticSegmentationLayer if semantic else TiledSegmentationLayer)(inner, case["tile_size"], case["overlap"], blend=case["blend"],
                                                                                    tile_batch_size=case["tile_batch_size"], accumulator_device="cpu")
    with torch.inference_mode():
        res = layer.predict(torch.from_numpy(frames)).pred_masks
    return torch.cat(tile_maps).numpy(), torch.cat(stitched).numpy(), res


def frame_margins(fg, hm, off, n_inst, min_inst):
    """``run_dir_case``'s checks on one frame's stitched maps: the uncertain set, or None when a margin is missed."""
    from sleap_nn.inference.segmentation import find_center_peaks

    t = torch.from_numpy(np.ascontiguousarray(hm[None, None]))
    peaks, vals = find_center_peaks(t, threshold=P["peak_threshold"], kernel_size=3)
    peaks, vals = peaks.numpy().reshape(-1, 2), np.sort(vals.numpy().astype(np.float64))
    if min_inst and not (0.10 <= float((fg > 0.5).mean()) <= 0.60 and 2 <= len(peaks) <= 40 and n_inst >= min_inst):
        return None
    if (len(vals) > 1 and np.diff(vals).min() < MARGIN) or (len(vals) and np.abs(vals - P["peak_threshold"]).min() < MARGIN):
        return None
    pooled = torch.nn.functional.max_pool2d(t, 3, 1, 1)[0, 0].numpy()
    cand = (hm >= pooled) & (hm > P["peak_threshold"])
    if cand.sum() != len(peaks):  # a plateau
        return None
    padded = np.pad(hm, 1, constant_values=-np.inf)
    second = np.full_like(hm, -np.inf)
    for dy in range(3):
        for dx in range(3):
            if (dy, dx) != (1, 1):
                second = np.maximum(second, padded[dy : dy + hm.shape[0], dx : dx + hm.shape[1]])
    if (cand.any() and (hm - second)[cand].min() < MARGIN) or ((second - hm)[~cand & (hm > P["peak_threshold"] - MARGIN)] < MARGIN).any():
        return None
    unc = np.abs(fg - 0.5) < MARGIN
    if len(peaks) >= 2:
        s = 2
        ys, xs = np.mgrid[0 : hm.shape[0], 0 : hm.shape[1]]
        px = xs * s + s / 2.0 + off[0].astype(np.float64)
        py = ys * s + s / 2.0 + off[1].astype(np.float64)
        cx, cy = peaks[:, 0] * s + s / 2.0, peaks[:, 1] * s + s / 2.0
        d = np.sort((px[..., None] - cx) ** 2 + (py[..., None] - cy) ** 2, axis=-1)
        unc = unc | ((fg > 0.5 - MARGIN) & (d[..., 1] - d[..., 0] < MARGIN * d[..., 1]))
    return unc if unc.mean() <= 0.005 else None


def record(out, prefix, case, frames, tiles, stitched, res, uncertain, seed):
    out[f"{prefix}/frames"], out[f"{prefix}/tiles"], out[f"{prefix}/stitched"], out[f"{prefix}/uncertain"] = frames, tiles, stitched, np.stack(uncertain)
    out[f"{prefix}/params"] = np.array(json.dumps(dict(P, seed=seed, **{k: v for k, v in case.items() if k != "min_inst"})))
    for b in range(len(res)):
        out[f"{prefix}/{b}/n"] = np.array(len(res[b]))
        out[f"{prefix}/{b}/scores"] = np.array([d["score"] for d in res[b]], dtype=np.float64)
        out[f"{prefix}/{b}/scales"] = np.array([d["scale"] for d in res[b]], dtype=np.float64).reshape(-1, 2)
        h, w = stitched.shape[-2:]
        out[f"{prefix}/{b}/masks"] = np.stack([d["mask"] for d in res[b]]) if len(res[b]) else np.zeros((0, h, w), dtype=bool)


def bottomup_cases(bu, sem):
    out, qualified = {}, {}
    for name, case in BU_CASES.items():
        good = []
        for seed in range(SEEDS):
            frames = frames_for(100 + seed, case["F"], case["H"], case["W"])
            tiles, stitched, res = run_reference(bu, frames, case, semantic=False)
            unc = [frame_margins(stitched[b, 0], stitched[b, 1], stitched[b, 2:4], len(res[b]), case["min_inst"]) for b in range(case["F"])]
            if any(u is None for u in unc):
                continue
            good.append(seed)
            if len(good) == 1:
                record(out, f"bu/{name}", case, frames, tiles, stitched, res, unc, 100 + seed)
                print(f"bu[{name}]: seed {100 + seed}, tiles {tiles.shape}, stitched {stitched.shape}, instances {[len(r) for r in res]}, "
                      f"fg {[round(float((stitched[b, 0] > 0.5).mean()), 3) for b in range(case['F'])]}, uncertain {[float(u.mean()) for u in unc]}")
                if name != "tiny":  # the semantic twin on the same frames: the one head is the same foreground
                    s_tiles, s_stitched, s_res = run_reference(sem, frames, case, semantic=True)
                    s_unc = [np.abs(s_stitched[b, 0] - 0.5) < MARGIN for b in range(case["F"])]
                    assert max(float(u.mean()) for u in s_unc) <= 0.005 and all(len(r) == 1 for r in s_res)
                    # same backbone, same head, same frames: the one head IS channel 0 of the bottom-up arrays, bit for bit.  Asserted here and not stored twice
                    # (the file stays under the size limit for committed files): readers take frames / tiles[:, :1] / stitched[:, :1] from ``bu/<case>``.
                    assert np.array_equal(s_tiles, tiles[:, :1]) and np.array_equal(s_stitched, stitched[:, :1]), "the semantic head is not the bottom-up foreground"
                    record(out, f"sem/{name}", case, frames, s_tiles, s_stitched, s_res, s_unc, 100 + seed)
                    for dup in ("frames", "tiles", "stitched"):
                        del out[f"sem/{name}/{dup}"]
                    print(f"sem[{name}]: fg range {float(s_stitched.min()):.3f} - {float(s_stitched.max()):.3f}, uncertain {[float(u.mean()) for u in s_unc]}")
                break
        assert good, f"no frame seed met the margins for {name}"
        qualified[name] = good
    out["bu/names"] = np.array(json.dumps(list(BU_CASES)))
    out["sem/names"] = np.array(json.dumps([n for n in BU_CASES if n != "tiny"]))
    return out


MERGER_CASES = {  # name -> (canvas (h, w), tile side, y origins, x origins, blend)
    "odd": ((45, 67), 16, [0, 13, 29], [0, 13, 26, 39, 51], "gaussian"),
    "vec": ((44, 68), 16, [0, 14, 28], [0, 13, 26, 39, 52], "pyramid"),
}


def merger_cases():
    from sleap_nn.inference.tile_merger import TileMerger, build_importance_window

    out = {}
    for i, (name, (hw, t, ys, xs, blend)) in enumerate(MERGER_CASES.items()):
        g = torch.Generator().manual_seed(700 + i)
        tiles = torch.randn((len(ys) * len(xs), 4, t, t), generator=g)
        win = build_importance_window((t, t), mode=blend)
        merger = TileMerger(hw, 4, win, device="cpu")
        for k, (y0, x0) in enumerate((y0, x0) for y0 in ys for x0 in xs):
            merger.integrate(tiles[k], y0, x0)
        merged = merger.merge()
        assert torch.isfinite(merged).all()
        out[f"merger/{name}/tiles"], out[f"merger/{name}/merged"] = tiles.numpy(), merged.numpy()
        out[f"merger/{name}/params"] = np.array(json.dumps(dict(hw=list(hw), tile=t, ys=ys, xs=xs, blend=blend)))
        print(f"merger[{name}]: {tuple(tiles.shape)} -> {tuple(merged.shape)}")
    out["merger/names"] = np.array(json.dumps(list(MERGER_CASES)))
    return out


def main():
    rh = gs.install()
    torch.set_num_threads(4)
    bu, sem = load_models(rh)
    gs.write_run_dir("tiny_tiled_semantic_segmentation", "semantic_segmentation", sem)
    arrs = {}
    arrs.update(bottomup_cases(bu, sem))
    arrs.update(merger_cases())
    p = os.path.join(GOLD, "tiled_segmentation.npz")
    np.savez_compressed(p, **arrs)
    print(f"wrote {p} ({os.path.getsize(p) / 1024:.0f} KiB, {len(arrs)} arrays)")


if __name__ == "__main__":
    main()
