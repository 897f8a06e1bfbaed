"""Generate the top-down segmentation goldens from the reference's own code (through ``oracle.ref_harness``, where the reference tree is available):

* ``tests/golden/topdown_segmentation.npz``
  - ``mask_layer/...``: synthetic logits in, the reference's ``CenteredInstanceMaskLayer.postprocess`` out (masks and scores);
  - ``layer/<case>/...``: the reference's ``TopDownSegmentationLayer`` over ``TorchBackend(cpu)`` on three 96 x 128 frames -- two with four bright blobs each
    (one within half a crop of the left and top edge, one within half a crop of the right and bottom edge) and one without a blob --, ``case`` = ``plain``
    (no sizematcher) and ``sized`` (``max_height`` / ``max_width`` that give ``eff`` < 1): mask, score, scale and offset of every entry, the sized crop
    corners and the uncertain set;
  - ``decode/<case>/...``: the reference's ``decode_mask_to_image_res`` on those entries.
* ``tests/golden/ckpt_dirs/tiny_centroid_seg`` (a centroid UNet) and ``tiny_centered_instance_segmentation`` (UNet, ``filters`` 8, crop 32 x 32, stride 2):
  ``best.ckpt`` (seeded weights saved here) + ``training_config.yaml``.

The harness does not stub ``lightning``; a stand-in (``LightningModule = torch.nn.Module``) is registered here before the reference modules are imported.
sleap-io is not installed: ``decode_mask_to_image_res`` gets a stand-in mask object with ``data``, ``scale``, ``offset``,
``image_extent = (round(h / sy), round(w / sx))`` and ``resampled(H, W)`` = ``F.interpolate(mode="nearest")``.  So the RESAMPLE RULE of ``decode/`` is pinned to
this stand-in, not to sleap-io itself (the same kind of stand-in as the SciPy one for OpenCV's ``erode`` in boundary IoU); everything after the resample
-- the rounding of the offset, the top-left pad, the dropped negative rows / columns -- is the reference's own code.

Margins asserted, the seed replaced when one fails: every centroid peak value is at least 1e-3 from the threshold; every sized centroid's
``top_left + half`` is at least 1e-2 from an integer, so the truncated crop origin cannot flip on the last bits of the refinement; crop probabilities within
1e-3 of ``fg_threshold`` are recorded as the uncertain set, at most 0.5 % of a crop's pixels.

    python tools/gen_topdown_seg_golden.py
"""
from __future__ import annotations

import json
import os
import sys
import types

import numpy as np
import torch
import yaml

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GOLD = os.path.join(ROOT, "tests", "golden")
MARGIN = 1e-3
CORNER_MARGIN = 1e-2
CROP, STRIDE, FG_THRESHOLD, PEAK_THRESHOLD, MAX_INSTANCES = 32, 2, 0.5, 0.2, 4
H, W = 96, 128
SIZED_MAX = (72, 96)  # eff = 0.75

BB = {"in_channels": 1, "kernel_size": 3, "filters": 8, "filters_rate": 2, "max_stride": 8, "stem_stride": None, "middle_block": True, "up_interpolate": True,
      "stacks": 1, "convs_per_block": 2, "output_stride": 2}
HEADS = {"centroid": {"confmaps": {"anchor_part": None, "sigma": 4.0, "output_stride": 2, "loss_weight": 1.0}},
         "centered_instance_segmentation": {"segmentation": {"output_stride": STRIDE, "loss_weight": 1.0, "anchor_part": None, "crop_size": CROP}}}
BLOBS = [[(8, 7), (119, 88), (50, 40), (90, 22)], [(10, 85), (118, 9), (40, 30), (84, 66)]]  # (x, y): corners first


def install():
    from oracle import ref_harness as rh

    rh.install()
    if "lightning" not in sys.modules:
        lm = types.ModuleType("lightning")
        lm.LightningModule = torch.nn.Module
        sys.modules["lightning"] = lm
    return rh


def frames(seed):
    g = np.random.default_rng(seed)
    fr = 30.0 + 3.0 * g.standard_normal((3, 1, H, W))
    yy, xx = np.mgrid[0:H, 0:W]
    for b, blobs in enumerate(BLOBS):
        for cx, cy in blobs:
            fr[b, 0] += g.uniform(170, 215) * np.exp(-((xx - cx) ** 2 + (yy - cy) ** 2) / (2 * g.uniform(4.5, 6.0) ** 2))
    return np.clip(fr, 0, 255).astype(np.uint8)


def seeded_model(rh, model_type, seed):
    from sleap_nn.architectures.model import Model

    torch.manual_seed(seed)
    m = Model("unet", rh.attrdict(BB), rh.attrdict(HEADS[model_type]), model_type).eval()
    with torch.no_grad():
        for _n, p in m.named_parameters():
            if p.dim() > 1:
                torch.nn.init.xavier_uniform_(p)
            else:
                p.uniform_(-0.1, 0.1)
    return m


def head_key(m, name):
    keys = [k for k in m.state_dict() if k.startswith("head_layers.0.") and k.endswith(name)]
    assert len(keys) == 1, keys
    return keys[0]


def fit_head(m, x, target, weight):
    """Least-squares fit of the 1x1 head on the seeded backbone's features: raw output ~ ``target`` where ``weight`` is set (maps at the head's resolution).
    The backbone stays the seeded random one; only the head's few numbers are chosen, so that the tiny models respond to the blobs."""
    head = m.head_layers[0]
    feats = {}
    hook = head.register_forward_hook(lambda _mod, inp, _out: feats.__setitem__("f", inp[0].detach()))
    with torch.no_grad():
        m(x)
    hook.remove()
    f = feats["f"].permute(0, 2, 3, 1).reshape(-1, feats["f"].shape[1]).double().numpy()
    sel = weight.reshape(-1)
    A = np.concatenate([f[sel], np.ones((int(sel.sum()), 1))], axis=1)
    sol = np.linalg.lstsq(A.T @ A + 1e-6 * np.eye(A.shape[1]), A.T @ target.reshape(-1)[sel].astype(np.float64), rcond=None)[0]
    wk, bk = head_key(m, ".0.weight"), head_key(m, ".0.bias")
    sd = m.state_dict()
    sd[wk] = torch.from_numpy(sol[:-1]).float().view_as(sd[wk])
    sd[bk] = torch.from_numpy(sol[-1:]).float().view_as(sd[bk])
    m.load_state_dict(sd)


def training_config(model_type, run_name, preprocessing):
    heads = {k: None for k in ("single_instance", "centroid", "centered_instance", "bottomup", "multi_class_bottomup", "multi_class_topdown",
                               "bottomup_segmentation", "semantic_segmentation", "centered_instance_segmentation")}
    heads[model_type] = HEADS[model_type]
    pre = {"ensure_rgb": False, "ensure_grayscale": True, "max_height": None, "max_width": None, "scale": 1.0, "crop_size": None}
    pre.update(preprocessing)
    return {"data_config": {"preprocessing": pre, "skeletons": []},
            "model_config": {"backbone_config": {"unet": BB, "convnext": None, "swint": None}, "head_configs": heads},
            "trainer_config": {"run_name": run_name}, "name": "", "description": "", "sleap_nn_version": "0.0.1"}


def write_run_dir(name, model_type, m, preprocessing):
    d = os.path.join(GOLD, "ckpt_dirs", name)
    os.makedirs(d, exist_ok=True)
    torch.save({"state_dict": {"model." + k: v.detach().clone() for k, v in m.state_dict().items()}}, os.path.join(d, "best.ckpt"))
    with open(os.path.join(d, "training_config.yaml"), "w") as f:
        yaml.safe_dump(training_config(model_type, name, preprocessing), f, sort_keys=False)
    print(f"wrote {d} ({os.path.getsize(os.path.join(d, 'best.ckpt')) / 1024:.0f} KiB)")


class StandInMask:
    """What ``decode_mask_to_image_res`` reads of a ``sio.SegmentationMask`` (module docstring: the resample rule is this stand-in's)."""

    def __init__(self, data, scale, offset):
        self.data, self.scale, self.offset = np.asarray(data, dtype=bool), tuple(scale), tuple(offset)

    @property
    def image_extent(self):
        h, w = self.data.shape
        return int(round(h / self.scale[1])), int(round(w / self.scale[0]))

    def resampled(self, height, width):
        t = torch.from_numpy(self.data).float()[None, None]
        out = torch.nn.functional.interpolate(t, size=(int(height), int(width)), mode="nearest")[0, 0].numpy() > 0.5
        return StandInMask(out, (1.0, 1.0), (0.0, 0.0))


def mask_layer_case():
    from sleap_nn.inference.layers.topdown_segmentation import CenteredInstanceMaskLayer

    g = np.random.default_rng(5)
    logits = (3.0 * g.standard_normal((5, 1, 16, 16))).astype(np.float32)
    logits[np.abs(logits) < 0.02] = 0.05  # (room around the threshold)
    logits[1] = -4.0  # an empty mask: score 0
    logits[2] = 4.0  # a full one
    probs = 1.0 / (1.0 + np.exp(-logits.astype(np.float64)))
    assert np.all(np.abs(probs - FG_THRESHOLD) >= MARGIN)
    layer = CenteredInstanceMaskLayer.__new__(CenteredInstanceMaskLayer)
    layer.fg_threshold = FG_THRESHOLD
    out = layer.postprocess({"SegmentationHead": torch.from_numpy(logits)}, None)
    # (the port's backend hands the layer PROBABILITIES: the sigmoid is recorded here with torch, as the reference's postprocess applies it)
    return {"mask_layer/logits": logits, "mask_layer/probs": torch.sigmoid(torch.from_numpy(logits)).numpy(), "mask_layer/masks": out.crops.numpy() > 0.5,
            "mask_layer/scores": out.instance_scores.numpy().astype(np.float64)}


def layer_cases(rh):
    import torch.nn as nn
    import torch.nn.functional as F

    import sleap_nn.data.resizing as rresizing
    from sleap_nn.inference.layers.backends.torch_backend import TorchBackend
    from sleap_nn.inference.layers.centroid import CentroidLayer
    from sleap_nn.inference.layers.configs import PostprocessConfig, PreprocessConfig
    from sleap_nn.inference.layers.topdown_segmentation import CenteredInstanceMaskLayer, TopDownSegmentationLayer
    from sleap_nn.inference.segmentation_convert import decode_mask_to_image_res

    class Fwd(nn.Module):  # the Lightning module's forward preamble: squeeze the n_samples axis, normalise; the seg module returns the head's logits
        def __init__(self, m, key):
            super().__init__()
            self.m, self.key = m, key

        def forward(self, x):
            x = torch.squeeze(x, dim=1)
            if x.dtype == torch.uint8 or x.max() > 1.0:
                x = x.float() / 255.0
            return self.m(x.float())[self.key]

    # torchvision is stubbed by the harness; the one call the sizematcher makes into it, transforms.v2.functional.resize on a tensor, is the torch operator
    # interpolate(bilinear, antialias=True) (as in oracle/gen_golden.py's sized top-down fixture)
    def tv_resize(image, size, **_kw):
        x = image if image.dim() == 4 else image[None]
        y = F.interpolate(x if x.dtype == torch.uint8 else x.float(), size=tuple(size), mode="bilinear", align_corners=False, antialias=True)
        return y if image.dim() == 4 else y[0]

    rresizing.tvf.resize = tv_resize
    yy, xx = np.mgrid[0 : H // 2, 0 : W // 2]
    for seed in range(300, 600):
        fr = frames(seed)
        x = torch.from_numpy(fr)
        xf = x.float() / 255
        target = np.zeros((3, H // 2, W // 2))
        for b, blobs in enumerate(BLOBS):
            for cx, cy in blobs:
                target[b] = np.maximum(target[b], 0.9 * np.exp(-((xx - cx / 2) ** 2 + (yy - cy / 2) ** 2) / (2 * 2.0**2)))
        mc = seeded_model(rh, "centroid", seed)
        fit_head(mc, xf, target, np.ones_like(target, dtype=bool))
        ms = seeded_model(rh, "centered_instance_segmentation", seed + 1000)
        bright = F.avg_pool2d(xf, 2).numpy()[:, 0]
        fit_head(ms, xf, np.where(bright > 0.35, 6.0, -6.0), (bright < 0.2) | (bright > 0.5))
        res, ok = {}, True
        for case, (mh, mw) in (("plain", (None, None)), ("sized", SIZED_MAX)):
            cl = CentroidLayer(TorchBackend(Fwd(mc, "CentroidConfmapsHead"), device="cpu"), 2, max_instances=MAX_INSTANCES, max_stride=BB["max_stride"],
                               preprocess_config=PreprocessConfig(ensure_grayscale=True, max_height=mh, max_width=mw),
                               postprocess_config=PostprocessConfig(peak_threshold=PEAK_THRESHOLD, max_instances=MAX_INSTANCES))
            il = CenteredInstanceMaskLayer(TorchBackend(Fwd(ms, "SegmentationHead"), device="cpu"), STRIDE, max_stride=BB["max_stride"], fg_threshold=FG_THRESHOLD)
            seen = {}
            inner = il.predict

            def spy(crops, _inner=inner, _seen=seen):
                _seen["crops"] = crops
                return _inner(crops)

            il.predict = spy
            td = TopDownSegmentationLayer(cl, il, (CROP, CROP))
            with torch.inference_mode():
                cout = cl.predict(x)
                out = td.predict(x)
                # every peak of the centroid maps (not only the kept ones) against the threshold
                xin, info = cl.preprocess(x)
                cms = cl.backend(xin)
                cms = cms["output"] if isinstance(cms, dict) else cms
            pooled = F.max_pool2d(cms, 3, 1, 1)
            cand = cms[(cms >= pooled)]
            cen, vals = cout.pred_centroids.numpy(), cout.pred_centroid_values.numpy()
            valid = ~np.isnan(cen[..., 0])
            n_per = valid.sum(1)
            if not (n_per[0] in (3, 4) and n_per[1] in (3, 4) and n_per[2] == 0) or "crops" not in seen:
                ok = False
                break
            if np.abs(cand.numpy() - PEAK_THRESHOLD).min() < MARGIN:
                ok = False
                break
            # no frame may hold more peaks than max_instances: the kept ones then stay in peak order, and no top-k decision rests on nearly equal values
            with torch.inference_mode():
                all_cl = CentroidLayer(cl.backend, 2, max_instances=None, max_stride=BB["max_stride"], preprocess_config=cl.preprocess_config,
                                       postprocess_config=PostprocessConfig(peak_threshold=PEAK_THRESHOLD))
                n_all = (~np.isnan(all_cl.predict(x).pred_centroids.numpy()[..., 0])).sum(1)
            if not np.array_equal(n_all, n_per):
                ok = False
                break
            crops = seen["crops"]
            if tuple(crops.shape[-2:]) != (CROP, CROP):  # (the reference sizes the gather by its first box in float32: one short for some centres)
                ok = False
                break
            eff = info.eff_scale.numpy().astype(np.float32)
            bi, si = np.nonzero(valid)
            sized = (torch.from_numpy(cen[bi, si]) * torch.from_numpy(eff[bi]).view(-1, 1)).numpy()
            topleft = np.stack([(sized[:, 0] - np.float32(CROP / 2)) + np.float32(0.5), (sized[:, 1] - np.float32(CROP / 2)) + np.float32(0.5)], axis=1).astype(np.float32)
            t = topleft + np.float32(CROP // 2)
            if np.abs(t - np.round(t)).min() < CORNER_MARGIN:
                ok = False
                break
            with torch.inference_mode():
                cin, _ = il.preprocess(crops)
                probs = torch.sigmoid(il.backend(cin)["output"]).numpy()[:, 0]
            unc = np.abs(probs - FG_THRESHOLD) < MARGIN
            frac = (probs > FG_THRESHOLD).reshape(len(probs), -1).mean(1)
            if unc.reshape(len(unc), -1).mean(1).max() > 0.005 or frac.min() < 0.05 or frac.max() > 0.9:
                ok = False
                break
            entries = [d for frame in out.pred_masks for d in frame]
            assert len(entries) == len(bi) and [len(f) for f in out.pred_masks] == n_per.tolist()
            offs = np.array([d["offset"] for d in entries])
            exts = np.array([StandInMask(d["mask"], d["scale"], d["offset"]).image_extent for d in entries])
            spill_tl = ((offs[:, 0] < -0.5) & (offs[:, 1] < -0.5)).any()
            spill_br = ((np.round(offs[:, 0]) + exts[:, 1] > W) & (np.round(offs[:, 1]) + exts[:, 0] > H)).any()
            if not (spill_tl and spill_br):
                ok = False
                break
            r = {f"layer/{case}/n": n_per.astype(np.int64), f"layer/{case}/eff": eff, f"layer/{case}/max_hw": np.array([mh or 0, mw or 0]),
                 f"layer/{case}/topleft_sized": topleft, f"layer/{case}/samples": bi.astype(np.int64), f"layer/{case}/uncertain": unc,
                 f"layer/{case}/masks": np.stack([d["mask"] for d in entries]), f"layer/{case}/scores": np.array([d["score"] for d in entries], dtype=np.float64),
                 f"layer/{case}/scales": np.array([d["scale"] for d in entries], dtype=np.float64), f"layer/{case}/offsets": offs.astype(np.float64)}
            for k, d in enumerate(entries):
                dec = decode_mask_to_image_res(StandInMask(d["mask"], d["scale"], d["offset"]))
                r[f"decode/{case}/{k}"] = np.asarray(dec, dtype=bool)
                # the stand-in's float32 nearest rule and the integer rule (u * w) // We of the port agree on these extents (asserted, not assumed)
                hh, ww = d["mask"].shape
                He, We = exts[k]
                rows, cols = (np.arange(He) * hh) // He, (np.arange(We) * ww) // We
                assert np.array_equal(StandInMask(d["mask"], d["scale"], d["offset"]).resampled(He, We).data, d["mask"][rows[:, None], cols[None, :]])
            res.update(r)
            print(f"seed {seed} {case}: entries {n_per.tolist()}, eff {eff.tolist()}, fg fraction {np.round(frac, 2).tolist()}, uncertain px {int(unc.sum())}, "
                  f"offsets {np.round(offs, 2).tolist()}, extents {exts.tolist()}")
        if not ok:
            continue
        res["layer/frames"] = fr
        res["layer/params"] = np.array(json.dumps({"seed": seed, "crop": CROP, "stride": STRIDE, "fg_threshold": FG_THRESHOLD, "peak_threshold": PEAK_THRESHOLD,
                                                   "max_instances": MAX_INSTANCES, "sized_max_hw": list(SIZED_MAX)}))
        write_run_dir("tiny_centroid_seg", "centroid", mc, {})
        write_run_dir("tiny_centered_instance_segmentation", "centered_instance_segmentation", ms, {"crop_size": CROP})
        return res
    raise AssertionError("no seed met the margins")


def main():
    rh = install()
    torch.set_num_threads(4)
    arrs = {}
    arrs.update(mask_layer_case())
    arrs.update(layer_cases(rh))
    p = os.path.join(GOLD, "topdown_segmentation.npz")
    np.savez_compressed(p, **arrs)
    print(f"wrote {p} ({os.path.getsize(p) / 1024:.0f} KiB, {len(arrs)} arrays)")


if __name__ == "__main__":
    main()
