"""Generate ``tests/golden/seg_training.npz`` from the reference's own code (through ``oracle.ref_harness`` and the ``lightning`` stand-in of
``tools/gen_segmentation_golden.py``, where the reference tree is available):

* ``losses/<case>/...``: inputs, and the value and autograd gradient of the reference's ``compute_bce_dice_loss`` / ``compute_masked_smooth_l1`` in fp32
  (``loss32``, ``grad32``) and evaluated in float64 (``loss64``, ``grad64``).
* ``targets/<case>/...``: ``masks`` (B, I, H, W) uint8 and ``n_instances`` in; per frame the reference's ``generate_foreground_mask``,
  ``generate_center_heatmap``, ``generate_center_offsets`` and ``_compute_mask_centroids`` out, called the way its dataset calls them
  (data/custom_datasets.py:3593-3626), stacked over the batch (centroids NaN in padding slots).
* ``step/bu`` and ``step/sem``: the weights of ``unet_tiny_seg.npz``, seeded images and masks, and the total loss, the per-head losses and every
  parameter gradient of the reference's own ``BottomUpSegmentationLightningModule.training_step`` / ``SemanticSegmentationLightningModule.training_step``
  (those configs have ``bce_weight = dice_weight = 1.0``, deliberately not the default).

Margins asserted so that no recorded decision sits on a rounding edge: no window at exactly half coverage (union or instance) except in the case that
tests it, and no two overlapping instances of equal area except in the tie case.

    python tools/gen_seg_training_golden.py
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
GOLD = os.path.join(ROOT, "tests", "golden")


# ---- (a) losses ---------------------------------------------------------------------------------------------------------------------------

def loss_cases():
    g = torch.Generator().manual_seed(101)
    cases = {}
    z = torch.randn((3, 1, 5, 7), generator=g) * 3.0
    t = (torch.rand((3, 1, 5, 7), generator=g) < 0.4).float()
    plant = [0.0, 30.0, -30.0, 80.0, -80.0]
    for k, v in enumerate(plant):  # each extreme against both target values
        z[0, 0, 0, k], t[0, 0, 0, k] = v, 0.0
        z[1, 0, 1, k], t[1, 0, 1, k] = v, 1.0
    for name, pw, bw, dw in (("bce_dice_default", None, 0.5, 0.5), ("bce_dice_pw3", 3.0, 1.0, 0.25)):
        cases[name] = dict(kind="bce_dice", pred=z.clone(), target=t.clone(), pos_weight=pw, bce_weight=bw, dice_weight=dw, smooth=1.0)
    cases["bce_dice_all_zero"] = dict(kind="bce_dice", pred=z.clone(), target=torch.zeros_like(t), pos_weight=None, bce_weight=0.5, dice_weight=0.5, smooth=1.0)
    cases["bce_dice_all_one"] = dict(kind="bce_dice", pred=z.clone(), target=torch.ones_like(t), pos_weight=3.0, bce_weight=0.5, dice_weight=0.5, smooth=1.0)
    p = torch.randn((2, 2, 6, 9), generator=g) * 1.5
    y = torch.randn((2, 2, 6, 9), generator=g) * 1.5
    p[0, 0, 0, 0], y[0, 0, 0, 0] = 0.75, -0.25  # a difference of exactly +1 (all four values exact in fp32) ...
    p[0, 1, 0, 1], y[0, 1, 0, 1] = -0.5, 0.5  # ... and of exactly -1
    p[0, 0, 0, 2], y[0, 0, 0, 2] = 2.5, 1.5
    p[0, 0, 0, 3], y[0, 0, 0, 3] = -0.25, 0.75
    m = (torch.rand((2, 1, 6, 9), generator=g) < 0.6).float()
    m[0, 0, 0, :4] = 1.0
    cases["sl1_mixed"] = dict(kind="sl1", pred=p.clone(), target=y.clone(), mask=m.clone())
    cases["sl1_empty_mask"] = dict(kind="sl1", pred=p.clone(), target=y.clone(), mask=torch.zeros_like(m))
    one = torch.zeros_like(m)
    one[1, 0, 3, 4] = 1.0
    cases["sl1_one_pixel"] = dict(kind="sl1", pred=p.clone(), target=y.clone(), mask=one)
    return cases


def run_loss_cases(ref_losses):
    out, names = {}, []
    for name, c in loss_cases().items():
        for dt, tag in ((torch.float32, "32"), (torch.float64, "64")):
            pred = c["pred"].clone().to(dt).requires_grad_(True)
            if c["kind"] == "bce_dice":
                loss = ref_losses.compute_bce_dice_loss(pred, c["target"].to(dt), bce_weight=c["bce_weight"], dice_weight=c["dice_weight"], smooth=c["smooth"],
                                                        pos_weight=c["pos_weight"])
            else:
                loss = ref_losses.compute_masked_smooth_l1(pred, c["target"].to(dt), c["mask"].to(dt))
            grad = torch.autograd.grad(loss, pred, allow_unused=True)[0]
            out[f"losses/{name}/loss{tag}"] = loss.detach().numpy()
            out[f"losses/{name}/grad{tag}"] = (torch.zeros_like(pred) if grad is None else grad).detach().numpy()
        for k in ("pred", "target", "mask"):
            if k in c:
                out[f"losses/{name}/{k}"] = c[k].numpy()
        out[f"losses/{name}/params"] = np.array(json.dumps({k: v for k, v in c.items() if not torch.is_tensor(v)}))
        names.append(name)
        print(f"loss[{name}]: {float(out[f'losses/{name}/loss32']):.7g} (fp64 {float(out[f'losses/{name}/loss64']):.12g})")
    out["losses/names"] = np.array(json.dumps(names))
    return out


# ---- (b) targets --------------------------------------------------------------------------------------------------------------------------

def disk(H, W, cx, cy, r):
    yy, xx = np.mgrid[0:H, 0:W]
    return ((xx - cx) ** 2 + (yy - cy) ** 2 <= r * r).astype(np.uint8)


def rect(H, W, y0, y1, x0, x1):
    m = np.zeros((H, W), np.uint8)
    m[y0:y1, x0:x1] = 1
    return m


def fix_half(frame, strides):
    """Grow the masks of a frame, one pixel at a time, until no window of these strides is covered to exactly one half, by one instance or by the union."""
    frame = [m.copy() for m in frame]
    for _ in range(500):
        changed = False
        for s in strides:
            H, W = frame[0].shape
            h, w = H // s, W // s
            union = np.zeros((H, W), np.uint8)
            for m in frame:
                union |= (m > 0).astype(np.uint8)
            for m in frame + [union]:
                cnt, size = window_counts((m > 0).astype(np.int64), h, w)
                for i, j in zip(*np.nonzero((2 * cnt == size) & (cnt > 0))):
                    y0, y1, x0, x1 = (i * H) // h, -((-(i + 1) * H) // h), (j * W) // w, -((-(j + 1) * W) // w)
                    tgt = m if m is not union else next(q for q in frame if q[y0:y1, x0:x1].any())
                    ys, xs = np.nonzero(union[y0:y1, x0:x1] == 0) if m is union else np.nonzero(m[y0:y1, x0:x1] == 0)
                    tgt[y0 + ys[0], x0 + xs[0]] = 1
                    changed = True
                if changed:
                    break
            if changed:
                break
        if not changed:
            return frame
    raise AssertionError("fix_half did not converge")


def target_cases():
    """name -> dict(frames = list of lists of (H, W) uint8 masks, I, stride, sigma, maxpool, allow_half, allow_tie, garbage)."""
    cases = {}

    def add(name, frames, stride, sigma=4.0, maxpool=False, I=None, allow_half=False, allow_tie=False, garbage=False):
        cases[name] = dict(frames=frames, stride=stride, sigma=sigma, maxpool=maxpool, I=I if I is not None else max(1, max(len(f) for f in frames)),
                           allow_half=allow_half, allow_tie=allow_tie, garbage=garbage)

    H, W = 40, 56
    blobs = fix_half([disk(H, W, 14.3, 12.1, 7.6), disk(H, W, 39.7, 25.2, 9.3), disk(H, W, 24.2, 30.4, 4.7)], (2, 4))
    for s in (1, 2, 4):
        add(f"blobs_s{s}", [blobs], s)
    add("nonuniform_10x13_s4", [[rect(10, 13, 1, 8, 2, 9), rect(10, 13, 5, 10, 8, 13)]], 4, sigma=1.5)
    add("big_70x150_s1", [[disk(70, 150, 40.2, 30.3, 17.4), disk(70, 150, 110.6, 41.8, 21.7), rect(70, 150, 3, 9, 120, 149)]], 1, sigma=2.0)
    add("batch_0_and_3", [[], blobs], 2)
    add("empty_real_mask", [[blobs[0], np.zeros((H, W), np.uint8), blobs[1]]], 2)
    one = np.zeros((H, W), np.uint8)
    one[21, 33] = 1
    add("one_pixel", [[one, blobs[0]]], 2)
    line = np.zeros((H, W), np.uint8)
    line[5:35, 27] = 1
    # (at stride 2 a straight one-pixel line covers exactly half of every cell it crosses; at stride 4 it covers a quarter: gone without maxpool, kept with it)
    add("line_s4", [[line, blobs[1]]], 4)
    add("line_s4_maxpool", [[line, blobs[1]]], 4, maxpool=True)
    add("line_s1", [[line, blobs[1]]], 1)
    halfm = rect(H, W, 10, 20, 10, 21)  # its last column covers exactly half of the stride-2 cells it touches
    add("half_coverage", [[halfm]], 2, allow_half=True)
    nested = fix_half([disk(H, W, 28.0, 20.0, 15.2), disk(H, W, 30.5, 21.5, 6.1)], (2,))
    add("nested", [nested], 2)
    add("nested_small_first", [nested[::-1]], 2)
    add("equal_area_tie", [[rect(H, W, 8, 24, 10, 30), rect(H, W, 14, 30, 20, 40), blobs[2] * 0 + rect(H, W, 32, 38, 2, 8)]], 2, allow_tie=True)
    add("padding_garbage", [[blobs[0], blobs[2]], [blobs[1]]], 2, I=5, garbage=True)
    return cases


def window_counts(m, h, w):
    H, W = m.shape
    out = np.zeros((h, w), np.int64)
    size = np.zeros((h, w), np.int64)
    for i in range(h):
        y0, y1 = (i * H) // h, -((-(i + 1) * H) // h)
        for j in range(w):
            x0, x1 = (j * W) // w, -((-(j + 1) * W) // w)
            out[i, j] = m[y0:y1, x0:x1].sum()
            size[i, j] = (y1 - y0) * (x1 - x0)
    return out, size


def assert_margins(name, c):
    s = c["stride"]
    for frame in c["frames"]:
        if not frame:
            continue
        H, W = frame[0].shape
        h, w = H // s, W // s
        union = np.zeros((H, W), np.uint8)
        covers = []
        for m in frame:
            union |= (m > 0).astype(np.uint8)
            cnt, size = window_counts((m > 0).astype(np.int64), h, w)
            half = 2 * cnt == size
            assert c["allow_half"] or not half.any(), (name, "an instance window at exactly half coverage")
            covers.append(2 * cnt > size)
        cnt, size = window_counts(union.astype(np.int64), h, w)
        assert c["allow_half"] or not (2 * cnt == size).any(), (name, "a union window at exactly half coverage")
        if c["allow_half"]:
            assert (2 * cnt == size).any(), (name, "the half-coverage case has no window at exactly half")
        areas = [int((m > 0).sum()) for m in frame]
        tie = False
        for a in range(len(frame)):
            for b in range(a + 1, len(frame)):
                if areas[a] == areas[b] and (covers[a] & covers[b]).any():
                    tie = True
        assert c["allow_tie"] or not tie, (name, "two overlapping instances of equal area")
        if c["allow_tie"]:
            assert tie, (name, "the tie case has no overlapping pair of equal area")


def run_target_cases(ref_maps):
    out, names = {}, []
    for name, c in target_cases().items():
        assert_margins(name, c)
        frames, I, s = c["frames"], c["I"], c["stride"]
        H, W = next(m.shape for f in frames for m in f)
        B = len(frames)
        g = np.random.default_rng(sum(name.encode()))
        masks = np.zeros((B, I, H, W), np.uint8)
        if c["garbage"]:
            masks[:] = (g.random((B, I, H, W)) < 0.5) * g.integers(1, 256, size=(B, I, H, W))
        n_inst = np.array([len(f) for f in frames], np.int32)
        fg, hm, off, wt = [], [], [], []
        cent = np.full((B, I, 2), np.nan, np.float32)
        for b, f in enumerate(frames):
            for i, m in enumerate(f):
                masks[b, i] = m * (1 if (b + i) % 2 == 0 else 255)  # non-zero = foreground, whatever the value
            mask_t = torch.from_numpy(masks[b : b + 1, : len(f)].astype(np.float32))
            arrays = [mask_t[0, k].numpy() > 0.5 for k in range(mask_t.shape[1])]
            centers = ref_maps._compute_mask_centroids(arrays) if arrays else []
            fg.append(ref_maps.generate_foreground_mask(arrays, img_hw=(H, W), output_stride=s, maxpool=c["maxpool"]))
            hm.append(ref_maps.generate_center_heatmap(arrays, img_hw=(H, W), output_stride=s, sigma=c["sigma"], centers=centers))
            o, wm = ref_maps.generate_center_offsets(arrays, img_hw=(H, W), output_stride=s, centers=centers)
            off.append(o)
            wt.append(wm)
            for i, (cx, cy) in enumerate(centers):
                cent[b, i] = torch.tensor([cx, cy], dtype=torch.float64).to(torch.float32).numpy()  # what fp32 torch arithmetic makes of the Python floats
        p = f"targets/{name}/"
        out[p + "masks"] = masks
        out[p + "n_instances"] = n_inst
        out[p + "foreground"] = torch.cat(fg).numpy()
        out[p + "center"] = torch.cat(hm).numpy()
        out[p + "offsets"] = torch.cat(off).numpy()
        out[p + "weight"] = torch.cat(wt).numpy()
        out[p + "centroids"] = cent
        out[p + "params"] = np.array(json.dumps({"stride": s, "sigma": c["sigma"], "maxpool": c["maxpool"]}))
        names.append(name)
        print(f"targets[{name}]: masks {masks.shape}, n {n_inst.tolist()}, fg {int(out[p + 'foreground'].sum())} cells, weight {int(out[p + 'weight'].sum())} cells")
    out["targets/names"] = np.array(json.dumps(names))
    return out


# ---- (c) training steps -------------------------------------------------------------------------------------------------------------------

def step_masks(seed, B, H, W, n_per_frame):
    g = np.random.default_rng(seed)
    I = max(n_per_frame)
    masks = np.zeros((B, I, H, W), np.uint8)
    for b in range(B):
        for i in range(n_per_frame[b]):
            masks[b, i] = disk(H, W, g.uniform(8, W - 8), g.uniform(8, H - 8), g.uniform(4.5, 9.5))
        masks[b, : n_per_frame[b]] = np.stack(fix_half(list(masks[b, : n_per_frame[b]]), (2,)))
    return masks, np.array(n_per_frame, np.int32)


def import_lightning_modules(rh):
    """The reference's Lightning modules import plotting and config packages that only their visualisation and setup code uses: every THIRD-PARTY
    module that is missing gets an inert stand-in (as the harness does for the ones it knows); the reference's own modules run unmodified."""
    import importlib

    if not hasattr(sys.modules["sleap_nn"], "__version__"):  # (the harness's namespace shim has none; a config default reads it)
        sys.modules["sleap_nn"].__version__ = "0.0.0"
    for _ in range(40):
        try:
            return importlib.import_module("sleap_nn.training.lightning_modules")
        except ModuleNotFoundError as e:
            name = e.name or ""
            if not name or name.split(".")[0] == "sleap_nn":
                raise
            m = rh._AnyModule(name)
            m.__path__ = []
            sys.modules[name] = m
            par, _, ch = name.rpartition(".")
            if par in sys.modules:
                setattr(sys.modules[par], ch, m)
            for k in [k for k in sys.modules if k.startswith("sleap_nn.training.lightning_modules") or k == "sleap_nn.training.utils"]:
                del sys.modules[k]
            print(f"(stand-in for the missing third-party module {name})")
    raise AssertionError("too many missing modules")


def run_steps(rh, ref_maps):
    lm = import_lightning_modules(rh)
    from sleap_nn.architectures.model import Model

    import gen_segmentation_golden as gs

    z = np.load(os.path.join(GOLD, "unet_tiny_seg.npz"))
    out = {}
    for prefix, cls in (("bu", lm.BottomUpSegmentationLightningModule), ("sem", lm.SemanticSegmentationLightningModule)):
        cfg = json.loads(str(z[f"{prefix}/config_json"]))
        mt = cfg["model_type"]
        heads = rh.attrdict({mt: cfg["heads"]})
        model = Model("unet", rh.attrdict(cfg["backbone"]), heads[mt], mt)
        model.load_state_dict({k[len(prefix) + 3 :]: torch.from_numpy(z[k]) for k in z.files if k.startswith(f"{prefix}/w/")}, strict=True)
        model.train()
        mod = cls.__new__(cls)
        torch.nn.Module.__init__(mod)
        mod.model, mod.model_type, mod.head_configs = model, mt, heads
        seg = heads[mt].segmentation
        mod.fg_bce_weight, mod.fg_dice_weight = getattr(seg, "bce_weight", 0.5), getattr(seg, "dice_weight", 0.5)
        mod.fg_bce_pos_weight = seg.get("bce_pos_weight", None)
        assert mod.fg_bce_weight == 1.0 and mod.fg_dice_weight == 1.0, "the tiny configs carry non-default loss weights on purpose"
        logged = {}
        mod.log = lambda name, value, **kw: logged.__setitem__(name, float(value))
        mod._accumulate_loss = lambda loss: None
        B, H, W = 2, 40, 56
        g = torch.Generator().manual_seed(77 + len(prefix))
        img = torch.randint(0, 256, (B, 1, 1, H, W), dtype=torch.uint8, generator=g)
        masks, n_inst = step_masks(300 + len(prefix), B, H, W, [3, 2])
        batch = {"image": img}
        keys = ("foreground_mask", "center_heatmap", "center_offsets", "foreground_weight")
        per = {k: [] for k in keys}
        for b in range(B):
            arrays = [masks[b, k] > 0 for k in range(n_inst[b])]
            centers = ref_maps._compute_mask_centroids(arrays)
            per["foreground_mask"].append(ref_maps.generate_foreground_mask(arrays, img_hw=(H, W), output_stride=seg.output_stride))
            if prefix == "bu":
                per["center_heatmap"].append(ref_maps.generate_center_heatmap(arrays, img_hw=(H, W), output_stride=heads[mt].center.output_stride,
                                                                              sigma=heads[mt].center.sigma, centers=centers))
                o, wm = ref_maps.generate_center_offsets(arrays, img_hw=(H, W), output_stride=heads[mt].offsets.output_stride, centers=centers)
                per["center_offsets"].append(o)
                per["foreground_weight"].append(wm)
        for k in keys:
            if per[k]:
                batch[k] = torch.cat(per[k]).unsqueeze(1)  # (B, 1, c, h, w), as the DataLoader collates the dataset's (1, c, h, w) samples
        loss = cls.training_step(mod, batch, 0)
        loss.backward()
        p = f"step/{prefix}/"
        out[p + "image"] = img.squeeze(1).numpy()
        out[p + "masks"] = masks
        out[p + "n_instances"] = n_inst
        out[p + "loss"] = np.array(float(loss), np.float64)
        names = {"SegmentationHead": "train/fg_loss", "InstanceCenterHead": "train/center_loss", "CenterOffsetHead": "train/offset_loss"}
        for head, key in names.items():
            if key in logged:
                out[p + f"head_loss/{head}"] = np.array(logged[key], np.float64)
        if prefix == "sem":
            out[p + "head_loss/SegmentationHead"] = np.array(float(loss), np.float64)
        for k, v in model.named_parameters():
            out[p + f"grad/{k}"] = v.grad.detach().numpy()
        for k, v in batch.items():
            if k != "image":
                out[p + f"target/{k}"] = v.squeeze(1).numpy()
        print(f"step[{prefix}]: loss {float(loss):.7g}, logged {logged}")
    return out


def main():
    import gen_segmentation_golden as gs

    rh = gs.install()
    torch.set_num_threads(4)
    import sleap_nn.data.segmentation_maps as ref_maps
    import sleap_nn.training.losses as ref_losses

    arrs = {}
    arrs.update(run_loss_cases(ref_losses))
    arrs.update(run_target_cases(ref_maps))
    arrs.update(run_steps(rh, ref_maps))
    p = os.path.join(GOLD, "seg_training.npz")
    np.savez_compressed(p, **arrs)
    size = os.path.getsize(p)
    print(f"wrote {p} ({size / 1024:.0f} KiB, {len(arrs)} arrays)")
    assert size < 1_000_000, "the golden must stay under the committed-file limit"


if __name__ == "__main__":
    main()
