"""Generate the segmentation goldens from the reference's own code (through ``oracle.ref_harness``, where the reference tree is available):

* ``tests/golden/segmentation.npz``
  - ``group/<case>/...``: synthetic head maps in, the reference's ``find_center_peaks`` / ``group_instances_from_offsets`` results out (centres, scores,
    and the per-instance masks as ONE label map: the reference's masks are disjoint, which is asserted);
  - ``layer/<case>/...``: the reference's ``SegmentationLayer.postprocess`` / ``SemanticSegmentationLayer.postprocess`` on ``PreprocInfo``s with an original
    size that is no multiple of the stride, input scale 0.5 and an ``eff_scale`` below 1, with ``min_mask_area`` and ``full_res_masks``;
  - ``rundir/...``: the reference's ``SegmentationLayer`` over ``TorchBackend(cpu)`` on two small frames with the run directory below.
* ``tests/golden/unet_tiny_seg.npz``: a seeded tiny UNet of ``bottomup_segmentation`` (``bu/``) and one of ``semantic_segmentation`` (``sem/``), each in the
  form of the other ``unet_tiny_*.npz`` (``w/``, ``image``, ``out/``, ``config_json``); ``out/`` is the Lightning module's ``forward``: sigmoid applied to the
  foreground head (lightning_modules.py:3041-3050).
* ``tests/golden/ckpt_dirs/tiny_bottomup_segmentation`` and ``tiny_semantic_segmentation``: ``best.ckpt`` + ``training_config.yaml``.

The harness does not stub ``lightning``; a stand-in (``LightningModule = torch.nn.Module``) is registered here before the reference modules are imported.

Margins asserted so that no recorded decision can flip on the last bit: every foreground pixel's best and second-best squared distance differ by at least
1e-3 relative, peak values are at least 1e-3 from the threshold (but for the one candidate placed exactly AT it) and, wherever their order decides (top-k,
the run directory), distinct by 1e-3; fg is at least 1e-3 from ``fg_threshold``.  With the distance gate, d is asserted 1e-3 relative away from every radius
it is compared with.  For the run directory the pixels that miss the fg / distance margins are recorded as the uncertain set, which must be at most 0.5 % of
the pixels; a seed that misses is replaced.

    python tools/gen_segmentation_golden.py
"""
from __future__ import annotations

import json
import math
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


def install():
    from oracle import ref_harness as rh

    rh.install()
    if "lightning" not in sys.modules:
        lm = types.ModuleType("lightning")
        lm.LightningModule = torch.nn.Module
        sys.modules["lightning"] = lm
    return rh


# ---- synthetic head maps ----------------------------------------------------------------------------------------------------------------

def blob_maps(h, w, stride, centers, amps, radius, seed, sigma=1.5, noise=0.25):
    """Centre map: a Gaussian of its own amplitude per centre over a 0.02 floor; foreground: 0.9 inside a disk around each centre (nearest centre owns the
    pixel), 0.1 outside; offsets: towards the owner's centre in input pixels plus uniform noise of +-``noise`` strides, random elsewhere."""
    g = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    hm = np.full((h, w), 0.02)
    for (cx, cy), a in zip(centers, amps):
        hm = np.maximum(hm, a * np.exp(-((xx - cx) ** 2 + (yy - cy) ** 2) / (2 * sigma**2)))
    fg = np.full((h, w), 0.1)
    off = g.uniform(-3 * stride, 3 * stride, size=(2, h, w))
    if len(centers):
        d = np.stack([(xx - cx) ** 2 + (yy - cy) ** 2 for cx, cy in centers])
        own = d.argmin(0)
        inside = d.min(0) <= radius**2
        fg[inside] = 0.9
        c = np.asarray(centers, dtype=np.float64)
        off[0][inside] = ((c[own, 0] - xx) * stride + g.uniform(-noise, noise, size=(h, w)) * stride)[inside]
        off[1][inside] = ((c[own, 1] - yy) * stride + g.uniform(-noise, noise, size=(h, w)) * stride)[inside]
    return fg.astype(np.float32), hm.astype(np.float32), off.astype(np.float32)


def grid_centers(h, w, step, margin):
    pts = [(x, y) for y in range(margin, h - margin + 1, step) for x in range(margin, w - margin + 1, step)]
    return pts


def amps_for(n, lo=0.45, hi=0.95, seed=0):
    a = np.linspace(hi, lo, n)
    np.random.default_rng(seed).shuffle(a)
    return a.tolist()


def group_cases():
    """name -> (fg (B,1,h,w), hm, off, params)."""
    P = dict(fg_threshold=0.5, peak_threshold=0.2, output_stride=2, max_instances=None, center_nms_kernel=3, distance_gate_alpha=None, distance_gate_iters=3)
    cases = {}

    def add(name, frames, **kw):
        fg = np.stack([f[0] for f in frames])[:, None]
        hm = np.stack([f[1] for f in frames])[:, None]
        off = np.stack([f[2] for f in frames])
        cases[name] = (fg, hm, off, dict(P, **kw))

    c3 = [(9, 8), (30, 20), (44, 29)]
    add("odd_37x53", [blob_maps(37, 53, 2, c3, [0.9, 0.8, 0.7], 7, 1)])
    add("one_center", [blob_maps(37, 53, 2, [(25, 17)], [0.9], 9, 2)])
    many = grid_centers(96, 96, 10, 6)[:70]
    add("many_96x96", [blob_maps(96, 96, 2, many, amps_for(len(many)), 4.5, 3, sigma=1.2)])
    add("one_row", [blob_maps(1, 41, 2, [(6, 0), (20, 0), (33, 0)], [0.9, 0.8, 0.7], 5, 4)])
    empty_fg = blob_maps(24, 31, 2, [(8, 8), (20, 14)], [0.9, 0.8], 5, 5)
    empty_fg = (np.full_like(empty_fg[0], 0.1), empty_fg[1], empty_fg[2])
    no_center = blob_maps(24, 31, 2, [(8, 8), (20, 14)], [0.15, 0.12], 5, 6)
    add("batch3", [blob_maps(24, 31, 2, [(7, 9), (22, 12)], [0.9, 0.8], 5, 7), empty_fg, no_center])
    for s in (1, 4):
        add(f"stride{s}", [blob_maps(37, 53, s, c3, [0.9, 0.8, 0.7], 7, 8 + s)], output_stride=s)

    # plateaus, hand-placed on the 37 x 53 map: values per pixel (x, y)
    def plateau_frame(seed, pixels, centers):
        fg, hm, off = blob_maps(37, 53, 2, centers, [0.3] * len(centers), 6, seed)  # low Gaussians: the hand-placed tops decide
        for (x, y), v in pixels:
            hm[y, x] = v
        return fg, hm, off

    pl = [((10, 8), 0.81), ((11, 8), 0.81),  # two tied, side by side
          ((30, 10), 0.77), ((30, 11), 0.77),  # two tied, stacked
          ((20, 25), 0.73), ((21, 25), 0.73), ((21, 26), 0.73),  # an L of three
          ((40, 20), 0.69), ((41, 21), 0.69),  # two tied, touching only diagonally: two peaks (k = 3: each is its window's maximum)
          ((0, 30), 0.65), ((0, 31), 0.65), ((52, 5), 0.61), ((52, 6), 0.61)]  # plateaus on the left and right border
    pc = [(10, 8), (30, 10), (20, 25), (40, 20), (0, 30), (52, 5)]
    add("plateaus", [plateau_frame(20, pl, pc)])
    # a plateau whose larger member comes later in raster order, and a candidate exactly AT the threshold (0.25: exact in fp32), which the strict test excludes
    pl2 = [((10, 8), 0.80), ((11, 8), 0.82), ((30, 20), 0.25)]
    add("at_threshold", [plateau_frame(21, pl2, [(10, 8), (30, 20), (44, 29)])], peak_threshold=0.25)
    # two peaks two pixels apart: separate at k = 3, the lower one suppressed at k = 5
    near = [((20, 15), 0.85), ((22, 15), 0.75), ((21, 15), 0.4)]
    for k in (3, 5, 7):
        add(f"nms{k}", [plateau_frame(22, near, [(20, 15), (40, 25)])], center_nms_kernel=k)
    # (foreground only around the nine centres that survive the cut: pixels that point at a removed centre of the regular grid would sit exactly between kept ones)
    amps = amps_for(len(many))
    fg9, hm9, off9 = blob_maps(96, 96, 2, many, amps, 4.5, 3, sigma=1.2)
    top = [many[i] for i in np.argsort(amps)[::-1][:9]]
    yy, xx = np.mgrid[0:96, 0:96]
    fg9[np.min([(xx - cx) ** 2 + (yy - cy) ** 2 for cx, cy in top], axis=0) > 4.5**2] = 0.1
    add("max_instances", [(fg9, hm9, off9)], max_instances=9)
    add("max_instances_37x53", [blob_maps(37, 53, 2, c3, [0.7, 0.9, 0.8], 7, 1)], max_instances=2)

    # distance gate: strays far from their centre are removed; one tiny instance is emptied and dropped; a pixel returns in a later pass
    def gate_frame(seed):
        fg, hm, off = blob_maps(48, 64, 2, [(14, 14), (44, 30), (30, 40)], [0.9, 0.8, 0.7], 8, seed, noise=0.1)
        yy, xx = np.mgrid[0:48, 0:64]
        # strays: a far strip of foreground whose offsets point nowhere near a centre
        fg[2:4, 50:62] = 0.9
        off[:, 2:4, 50:62] = 0.0
        # the third instance keeps only 3 pixels, all pointing 5 px away from its centre: its radius cannot hold them
        third = (xx - 30) ** 2 + (yy - 40) ** 2 <= 64
        fg[third] = 0.1
        for (x, y) in ((30, 40), (31, 40), (30, 41)):
            fg[y, x] = 0.9
            off[0, y, x] = (30 - x) * 2 + 5.0
            off[1, y, x] = (40 - y) * 2
        return fg, hm, off

    add("gate", [gate_frame(30)], distance_gate_alpha=1.6)
    add("gate_shells", [gate_shells_frame()], distance_gate_alpha=1.0)
    add("gate_shells_2", [gate_shells_frame()], distance_gate_alpha=1.0, distance_gate_iters=2)
    pk = np.array([(x, y) for y in range(0, 96, 2) for x in range(0, 96, 2)], dtype=np.float64)
    for seed in range(50, 90):  # (random offsets among centres 4 px apart: a seed whose 400 pixels all clear the distance margin)
        fr = lattice_frame(seed)
        try:
            margins_ok(fr[0], fr[1], fr[2], P, pk)
        except AssertionError:
            continue
        add("lattice", [fr])
        break
    assert "lattice" in cases
    add("gate_batch", [gate_frame(31), blob_maps(48, 64, 2, [(20, 20)], [0.9], 9, 32)], distance_gate_alpha=2.0, distance_gate_iters=2)
    return cases


def gate_shells_frame():
    """One instance whose pixels sit in shells around its centre: 40 at distance 0, then 10 each at 9.5, 9.0 and 8.2 px (alpha 1, stride 2:
    r(70) = 9.44, r(60) = 8.74, r(50) = 7.98).  Pass 1 drops the outer shell, pass 2 the next, pass 3 the third: the result depends on the pass count.
    (A pixel cannot RETURN in a later pass: the first radius comes from all assigned pixels, so the kept counts, the radii and the kept sets can only
    shrink from pass to pass.  The kernels still recompute ``keep`` over all assigned pixels each pass, as the reference does.)  A second instance is the control."""
    h, w, s = 40, 56, 2
    fg = np.full((h, w), 0.1, np.float32)
    hm = np.full((h, w), 0.02, np.float32)
    off = np.zeros((2, h, w), np.float32)
    ca, cb = (12, 12), (40, 26)
    hm[ca[1], ca[0]], hm[cb[1], cb[0]] = 0.9, 0.8

    def put(x, y, c, dist_px):  # pixel (x, y) predicts a point dist_px to the right of centre c
        fg[y, x] = 0.9
        off[0, y, x] = (c[0] - x) * s + dist_px
        off[1, y, x] = (c[1] - y) * s

    cells = [(x, y) for y in range(4, 22) for x in range(2, 26)]
    for k, dist in enumerate([0.0] * 40 + [9.5] * 10 + [9.0] * 10 + [8.2] * 10):
        put(*cells[k], ca, dist)
    cells_b = [(x, y) for y in range(22, 32) for x in range(34, 50)]
    for k, dist in enumerate([0.0] * 3 + [3.2] * 30):
        put(*cells_b[k], cb, dist)
    return fg, hm, off


def lattice_frame(seed):
    """96 x 96 with a centre on every second pixel (2 304 centres: more than the LDS candidate list and more than one LDS chunk of centres) and a 20 x 20 block of foreground."""
    g = np.random.default_rng(seed)
    hm = np.full((96, 96), 0.02, np.float32)
    vals = 0.3 + 0.6 * (g.permutation(48 * 48) + 0.5) / (48 * 48)
    hm[0::2, 0::2] = vals.reshape(48, 48).astype(np.float32)
    fg = np.full((96, 96), 0.1, np.float32)
    fg[31:51, 40:60] = 0.9
    off = g.uniform(-6, 6, size=(2, 96, 96)).astype(np.float32)
    return fg, hm, off


def margins_ok(fg, hm, off, p, peaks):
    """Asserts the recorded decisions have room.  ``peaks``: the kept centres (N, 2) grid (x, y)."""
    s = p["output_stride"]
    assert np.all(np.abs(fg - p["fg_threshold"]) >= MARGIN), "fg too close to fg_threshold"
    m = fg > p["fg_threshold"]
    if len(peaks) >= 2 and m.any():
        ys, xs = np.nonzero(m)
        px = xs * s + s / 2.0 + off[0][ys, xs].astype(np.float64)
        py = ys * s + s / 2.0 + off[1][ys, xs].astype(np.float64)
        cx, cy = peaks[:, 0] * s + s / 2.0, peaks[:, 1] * s + s / 2.0
        dall = (px[:, None] - cx[None]) ** 2 + (py[:, None] - cy[None]) ** 2
        d = np.sort(dall, axis=1)
        assert np.all(d[:, 1] - d[:, 0] >= MARGIN * d[:, 1]), "best / second-best distance too close"
    if p["distance_gate_alpha"] is not None and len(peaks) and m.any():
        ys, xs = np.nonzero(m)
        px = xs * s + s / 2.0 + off[0][ys, xs].astype(np.float64)
        py = ys * s + s / 2.0 + off[1][ys, xs].astype(np.float64)
        dall = (px[:, None] - (peaks[:, 0] * s + s / 2.0)[None]) ** 2 + (py[:, None] - (peaks[:, 1] * s + s / 2.0)[None]) ** 2
        a, dmin = dall.argmin(1), dall.min(1)
        keep = np.ones(len(a), bool)
        for _ in range(max(1, p["distance_gate_iters"])):
            r2 = (p["distance_gate_alpha"] * np.sqrt(np.bincount(a[keep], minlength=len(peaks)) / math.pi) * s) ** 2
            assert np.all(np.abs(dmin - r2[a]) >= MARGIN * np.maximum(r2[a], 1e-30)), "d too close to a gate radius"
            keep = dmin <= r2[a]


def run_group_cases(ref_seg):
    out = {}
    names = []
    for name, (fg, hm, off, p) in group_cases().items():
        B = fg.shape[0]
        out[f"group/{name}/fg"], out[f"group/{name}/hm"], out[f"group/{name}/off"] = fg, hm, off
        out[f"group/{name}/params"] = np.array(json.dumps(p))
        for b in range(B):
            tf, th, to = (torch.from_numpy(a[b : b + 1]) for a in (fg, hm, off))
            peaks, vals = ref_seg.find_center_peaks(th, threshold=p["peak_threshold"], kernel_size=p["center_nms_kernel"])
            if p["max_instances"] is not None and len(peaks) > p["max_instances"]:
                vals, keep = torch.topk(vals, p["max_instances"])
                peaks = peaks[keep]
            peaks_np, vals_np = peaks.numpy().astype(np.int32).reshape(-1, 2), vals.numpy().astype(np.float32)
            if p["max_instances"] is not None:
                # distinct wherever their order decides: the top-k cases (the diagonal pair of the plateau case is tied by construction)
                all_vals = np.sort(ref_seg.find_center_peaks(th, threshold=p["peak_threshold"], kernel_size=p["center_nms_kernel"])[1].numpy().astype(np.float64))
                assert np.all(np.diff(all_vals) >= MARGIN), (name, "peak values not distinct")
            assert np.all(np.abs(vals_np - p["peak_threshold"]) >= MARGIN), (name, "peak value too close to the threshold")
            margins_ok(fg[b, 0], hm[b, 0], off[b], p, peaks_np.astype(np.float64))
            inst = ref_seg.group_instances_from_offsets(tf, th, to, fg_threshold=p["fg_threshold"], peak_threshold=p["peak_threshold"], output_stride=p["output_stride"],
                                                        max_instances=p["max_instances"], center_nms_kernel=p["center_nms_kernel"],
                                                        distance_gate_alpha=p["distance_gate_alpha"], distance_gate_iters=p["distance_gate_iters"])
            lab = np.full(fg.shape[-2:], -1, dtype=np.int16)
            for i, d in enumerate(inst):
                assert np.all(lab[d["mask"]] == -1), (name, "reference masks overlap")
                lab[d["mask"]] = i
            out[f"group/{name}/{b}/peaks"], out[f"group/{name}/{b}/peak_vals"] = peaks_np, vals_np
            out[f"group/{name}/{b}/labels"] = lab
            out[f"group/{name}/{b}/inst_centers"] = np.array([d["center"] for d in inst], dtype=np.float64).reshape(-1, 2)
            out[f"group/{name}/{b}/inst_scores"] = np.array([d["score"] for d in inst], dtype=np.float64)
            print(f"group[{name}][{b}]: {len(peaks_np)} centres, {len(inst)} instances, {(lab >= 0).sum()} px")
        names.append(name)
    out["group/names"] = np.array(json.dumps(names))
    return out


# ---- layer cases ------------------------------------------------------------------------------------------------------------------------

LAYER_INFOS = {
    # name -> (original (h, w), processed (h, w), eff_scale, input_scale, output_stride, map (h, w))
    "not_multiple": ((45, 61), (48, 64), 1.0, 1.0, 2, (24, 32)),
    "input_scale_half": ((90, 122), (48, 64), 1.0, 0.5, 2, (24, 32)),
    "eff_below_1": ((120, 160), (48, 64), 0.4, 1.0, 2, (24, 32)),
    "stride4_scale_half": ((100, 135), (64, 80), 1.0, 0.5, 4, (16, 20)),
    "no_metadata": ((0, 0), (0, 0), 1.0, 1.0, 2, (24, 32)),
}


def layer_maps(name, hw, stride):
    h, w = hw
    cs = [(5, 5), (w - 4, h - 4), (w // 2, h // 2)]  # one instance reaches the bottom-right corner: the crop matters
    fg, hm, off = blob_maps(h, w, stride, cs, [0.9, 0.8, 0.7], 4, 40 + sum(name.encode()) % 50, noise=0.1)
    fg[2, w - 2] = 0.9  # a lone pixel that joins some instance: the area floor decides on small masks
    return fg, hm, off


def run_layer_cases():
    from sleap_nn.inference.layers.configs import PostprocessConfig
    from sleap_nn.inference.layers.segmentation import SegmentationLayer, SemanticSegmentationLayer
    from sleap_nn.inference.preprocess_info import PreprocInfo

    out, names = {}, []
    for iname, (orig, proc, eff, iscale, stride, hw) in LAYER_INFOS.items():
        fg, hm, off = layer_maps(iname, hw, stride)
        for min_area in (0, 40, 250):
            for full in (False, True):
                for semantic in (False, True):
                    name = f"{iname}/a{min_area}/{'full' if full else 'stride'}/{'sem' if semantic else 'inst'}"
                    layer = (SemanticSegmentationLayer if semantic else SegmentationLayer).__new__(SemanticSegmentationLayer if semantic else SegmentationLayer)
                    layer.fg_threshold, layer.min_mask_area, layer.max_instances, layer.full_res_masks = 0.5, min_area, None, full
                    layer.output_stride, layer.postprocess_config = stride, PostprocessConfig(peak_threshold=0.2)
                    info = PreprocInfo(original_size=orig, processed_size=proc, eff_scale=torch.tensor([eff], dtype=torch.float32), input_scale=iscale, output_stride=stride)
                    raw = {"SegmentationHead": torch.from_numpy(fg)[None, None], "InstanceCenterHead": torch.from_numpy(hm)[None, None], "CenterOffsetHead": torch.from_numpy(off)[None]}
                    res = layer.postprocess(raw, info).pred_masks[0]
                    out[f"layer/{name}/n"] = np.array(len(res))
                    for i, d in enumerate(res):
                        out[f"layer/{name}/{i}/mask"] = np.asarray(d["mask"], dtype=bool)
                        out[f"layer/{name}/{i}/meta"] = np.array([d["score"], d["scale"][0], d["scale"][1], d["offset"][0], d["offset"][1]], dtype=np.float64)
                    names.append(name)
        out[f"layer/{iname}/fg"], out[f"layer/{iname}/hm"], out[f"layer/{iname}/off"] = fg, hm, off
    out["layer/names"] = np.array(json.dumps(names))
    out["layer/infos"] = np.array(json.dumps({k: [list(v[0]), list(v[1]), v[2], v[3], v[4], list(v[5])] for k, v in LAYER_INFOS.items()}))
    print(f"layer: {len(names)} cases")
    return out


# ---- models and run directories ---------------------------------------------------------------------------------------------------------

BB = {"in_channels": 1, "kernel_size": 3, "filters": 8, "filters_rate": 2, "max_stride": 8, "stem_stride": None, "middle_block": True, "up_interpolate": True,
      "stacks": 1, "convs_per_block": 2, "output_stride": 2}
HEADS = {"bottomup_segmentation": {"segmentation": {"output_stride": 2, "loss_weight": 1.0, "bce_weight": 1.0, "dice_weight": 1.0},
                                   "center": {"sigma": 4.0, "output_stride": 2, "loss_weight": 1.0}, "offsets": {"output_stride": 2, "loss_weight": 0.1}},
         "semantic_segmentation": {"segmentation": {"output_stride": 2, "loss_weight": 1.0, "bce_weight": 1.0, "dice_weight": 1.0}}}


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


def lightning_forward(m, x_uint8):
    """The Lightning module's forward (lightning_modules.py:3041-3050, 3450-3461): squeeze, normalise, model, sigmoid on the foreground head."""
    with torch.inference_mode():
        out = m(x_uint8.float() / 255)
    return {k: (torch.sigmoid(v) if k == "SegmentationHead" else v) for k, v in out.items()}


def tiny_models(rh):
    out = {}
    for prefix, mt, seed, hw in (("bu", "bottomup_segmentation", 61, (40, 56)), ("sem", "semantic_segmentation", 62, (40, 56))):
        m = seeded_model(rh, mt, seed)
        keys = list(m.state_dict().keys())
        g = torch.Generator().manual_seed(seed + 1)
        img = torch.randint(0, 256, (2, 1, 1, hw[0], hw[1]), dtype=torch.uint8, generator=g)
        res = lightning_forward(m, img.squeeze(1))
        for k, v in m.state_dict().items():
            out[f"{prefix}/w/{k}"] = v.detach().numpy()
        out[f"{prefix}/image"] = img.numpy()
        for k, v in res.items():
            out[f"{prefix}/out/{k}"] = v.numpy()
        out[f"{prefix}/config_json"] = np.array(json.dumps({"backbone": BB, "heads": HEADS[mt], "model_type": mt}))
        print(f"model[{mt}]: head keys {[k for k in keys if k.startswith('head_layers')]}")
    return out


def training_config(model_type, run_name):
    heads = {k: None for k in ("single_instance", "centroid", "centered_instance", "bottomup", "multi_class_bottomup", "multi_class_topdown",
                               "bottomup_segmentation", "semantic_segmentation")}
    heads[model_type] = HEADS[model_type]
    return {"data_config": {"preprocessing": {"ensure_rgb": False, "ensure_grayscale": True, "max_height": None, "max_width": None, "scale": 1.0, "crop_size": None},
                            "skeletons": []},
            "model_config": {"backbone_config": {"unet": BB, "convnext": None, "swint": None}, "head_configs": heads},
            "trainer_config": {"run_name": run_name}, "name": "", "description": "", "sleap_nn_version": "0.0.1"}


def write_run_dir(name, model_type, m):
    d = os.path.join(GOLD, "ckpt_dirs", name)
    os.makedirs(d, exist_ok=True)
    torch.save({"state_dict": {"model." + k: v.detach().clone() for k, v in m.state_dict().items()}}, os.path.join(d, "best.ckpt"))
    with open(os.path.join(d, "training_config.yaml"), "w") as f:
        yaml.safe_dump(training_config(model_type, name), f, sort_keys=False)
    return d


def run_dir_frames(seed):
    """Two 72 x 100 uint8 frames: a few bright disks on a dim textured background."""
    g = np.random.default_rng(seed)
    fr = np.zeros((2, 1, 72, 100), dtype=np.float64)
    yy, xx = np.mgrid[0:72, 0:100]
    for b in range(2):
        fr[b, 0] = 30 + 10 * g.standard_normal((72, 100))
        for _ in range(4):
            cx, cy, r = g.uniform(12, 88), g.uniform(12, 60), g.uniform(6, 11)
            fr[b, 0][(xx - cx) ** 2 + (yy - cy) ** 2 <= r * r] = g.uniform(150, 240)
    return np.clip(fr, 0, 255).astype(np.uint8)


def run_dir_case(rh):
    """Seeded weights + head biases such that the reference layer finds >= 2 well-separated centres per frame and 10-60 % foreground."""
    import torch.nn as nn

    from sleap_nn.inference.layers.backends.torch_backend import TorchBackend
    from sleap_nn.inference.layers.configs import PostprocessConfig, PreprocessConfig
    from sleap_nn.inference.layers.segmentation import SegmentationLayer

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

    P = dict(fg_threshold=0.5, peak_threshold=0.2, output_stride=2, center_nms_kernel=3)
    for seed in range(100, 160):
        m = seeded_model(rh, "bottomup_segmentation", seed)
        frames = run_dir_frames(seed)
        x = torch.from_numpy(frames)
        sd = m.state_dict()
        with torch.no_grad():
            raw = m(x.float() / 255)
            # head weights scaled so the maps have O(1) contrast, biases placed from the maps' own quantiles
            for i, (key, q, target, gain) in enumerate((("SegmentationHead", 0.65, 0.0, 8.0), ("InstanceCenterHead", 0.97, 0.2, 4.0))):
                wk, bk = f"head_layers.{i}.{key}.0.weight", f"head_layers.{i}.{key}.0.bias"
                v = raw[key]
                sd[wk] *= gain / float(v.std())
                sd[bk].fill_(0.0)
            m.load_state_dict(sd)
            raw = m(x.float() / 255)
            sd = m.state_dict()
            sd["head_layers.0.SegmentationHead.0.bias"] -= float(torch.quantile(raw["SegmentationHead"].flatten(), 0.65))
            sd["head_layers.1.InstanceCenterHead.0.bias"] += 0.2 - float(torch.quantile(raw["InstanceCenterHead"].flatten(), 0.97))
            m.load_state_dict(sd)
        layer = SegmentationLayer(TorchBackend(Fwd(m), device="cpu"), 2, max_stride=BB["max_stride"], preprocess_config=PreprocessConfig(ensure_grayscale=True),
                                  postprocess_config=PostprocessConfig(peak_threshold=P["peak_threshold"]))
        with torch.inference_mode():
            xin, info = layer.preprocess(x)
            raw = layer.backend(xin)
            res = layer.postprocess(raw, info).pred_masks
        fg, hm, off = (raw[k].numpy() for k in ("SegmentationHead", "InstanceCenterHead", "CenterOffsetHead"))
        ok, unc_frac, uncertain = True, [], []
        from sleap_nn.inference.segmentation import find_center_peaks

        for b in range(2):
            frac = float((fg[b, 0] > 0.5).mean())
            peaks, vals = find_center_peaks(torch.from_numpy(hm[b : b + 1]), threshold=P["peak_threshold"], kernel_size=3)
            peaks, vals = peaks.numpy().reshape(-1, 2), np.sort(vals.numpy().astype(np.float64))
            if not (0.10 <= frac <= 0.60 and 2 <= len(peaks) <= 40 and len(res[b]) >= 2):
                ok = False
                break
            if (len(vals) > 1 and np.diff(vals).min() < MARGIN) or np.abs(vals - P["peak_threshold"]).min() < MARGIN:
                ok = False
                break
            # the candidate structure itself must have room: a candidate clears every other value of its window by MARGIN, and every other pixel above
            # (threshold - MARGIN) stays MARGIN below its window maximum
            t = torch.from_numpy(hm[b : b + 1])
            pooled = torch.nn.functional.max_pool2d(t, 3, 1, 1)[0, 0].numpy()
            h0 = hm[b, 0]
            cand = (h0 >= pooled) & (h0 > P["peak_threshold"])
            if cand.sum() != len(peaks):  # a plateau
                ok = False
                break
            padded = np.pad(h0, 1, constant_values=-np.inf)
            second = np.full_like(h0, -np.inf)
            for dy in range(3):
                for dx in range(3):
                    if (dy, dx) != (1, 1):
                        second = np.maximum(second, padded[dy : dy + h0.shape[0], dx : dx + h0.shape[1]])
            if (h0 - second)[cand].min() < MARGIN or ((second - h0)[~cand & (h0 > P["peak_threshold"] - MARGIN)] < MARGIN).any():
                ok = False
                break
            s = 2
            ys, xs = np.mgrid[0 : h0.shape[0], 0 : h0.shape[1]]
            px = xs * s + s / 2.0 + off[b, 0].astype(np.float64)
            py = ys * s + s / 2.0 + off[b, 1].astype(np.float64)
            cx, cy = peaks[:, 0] * s + s / 2.0, peaks[:, 1] * s + s / 2.0
            d = np.sort((px[..., None] - cx) ** 2 + (py[..., None] - cy) ** 2, axis=-1)
            unc = (np.abs(fg[b, 0] - 0.5) < MARGIN) | ((fg[b, 0] > 0.5 - MARGIN) & (d[..., 1] - d[..., 0] < MARGIN * d[..., 1]))
            unc_frac.append(float(unc.mean()))
            uncertain.append(unc)
            if unc.mean() > 0.005:
                ok = False
                break
        if not ok:
            continue
        assert max(unc_frac) <= 0.005
        write_run_dir("tiny_bottomup_segmentation", "bottomup_segmentation", m)
        out = {"rundir/frames": frames, "rundir/uncertain": np.stack(uncertain), "rundir/params": np.array(json.dumps(dict(P, seed=seed)))}
        for b in range(2):
            out[f"rundir/{b}/n"] = np.array(len(res[b]))
            out[f"rundir/{b}/scores"] = np.array([d["score"] for d in res[b]], dtype=np.float64)
            out[f"rundir/{b}/scales"] = np.array([d["scale"] for d in res[b]], dtype=np.float64).reshape(-1, 2)
            out[f"rundir/{b}/masks"] = np.stack([d["mask"] for d in res[b]])
        print(f"rundir: seed {seed}, instances {[len(r) for r in res]}, fg {[round(float((fg[b, 0] > 0.5).mean()), 3) for b in range(2)]}, uncertain {unc_frac}")
        write_run_dir("tiny_semantic_segmentation", "semantic_segmentation", seeded_model(rh, "semantic_segmentation", seed))
        return out
    raise AssertionError("no seed met the run-directory margins")


def main():
    rh = install()
    torch.set_num_threads(4)
    import sleap_nn.inference.segmentation as ref_seg

    arrs = {}
    arrs.update(run_group_cases(ref_seg))
    arrs.update(run_layer_cases())
    arrs.update(run_dir_case(rh))
    p = os.path.join(GOLD, "segmentation.npz")
    np.savez_compressed(p, **arrs)
    print(f"wrote {p} ({os.path.getsize(p) / 1024:.0f} KiB, {len(arrs)} arrays)")
    p = os.path.join(GOLD, "unet_tiny_seg.npz")
    np.savez_compressed(p, **tiny_models(rh))
    print(f"wrote {p} ({os.path.getsize(p) / 1024:.0f} KiB)")


if __name__ == "__main__":
    main()
