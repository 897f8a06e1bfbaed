"""Generate ``tests/golden/seg_cleanup.npz`` from the reference's own code (through ``oracle.ref_harness`` and the ``lightning`` stand-in of
``tools/gen_segmentation_golden.py``, where the reference tree and SciPy are available): ``group_instances_from_offsets(mask_cleanup=True)`` and
``SegmentationLayer.postprocess`` with ``mask_cleanup`` on.

* ``group/<case>/...``: head maps in; per frame the reference's centres and, per instance, its cleaned mask, centre and score.  Cleaned masks overlap (a
  ring fills over what it encloses), so they are recorded one by one, not as a label map.
* ``layer/<case>/...``: the reference layer's ``pred_masks`` with ``min_mask_area`` on a map where the cleanup moves instances across the floor.
* ``rundir/...``: the reference ``SegmentationLayer(mask_cleanup=True)`` over ``TorchBackend(cpu)`` with the weights of
  ``tests/golden/ckpt_dirs/tiny_bottomup_segmentation`` on two frames.  A flipped pixel can change connectivity, so the frames' seed is chosen such that the
  uncertain set (pixels that miss the fg / distance margins) is EMPTY, which is asserted; the peaks clear the margins of the uncleaned generator as well.

Most cases are painted label maps: every foreground pixel's offset points exactly at its centre (d = 0 against at least one stride for any other centre), fg
is 0.9 / 0.1 and each centre is a lone pixel of its own amplitude, so every margin of the uncleaned generator (1e-3 from each threshold, asserted again here
through its ``margins_ok``) holds trivially and the label map is stable on the last bit.  Cleanup itself is integer work: exact.

    python tools/gen_seg_cleanup_golden.py
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
import gen_segmentation_golden as base  # noqa: E402

GOLD = base.GOLD
MARGIN = base.MARGIN
P0 = dict(fg_threshold=0.5, peak_threshold=0.2, output_stride=2, max_instances=None, center_nms_kernel=3, distance_gate_alpha=None, distance_gate_iters=3)


def paint(lab, centers, stride=2):
    """``lab`` (h, w) int, -1 = background, k = the k-th centre; ``centers`` [(x, y)] in raster order, lone pixels at least two apart."""
    h, w = lab.shape
    assert all(b[1] * w + b[0] > a[1] * w + a[0] for a, b in zip(centers, centers[1:])), "centres must come in raster order"
    for i, a in enumerate(centers):
        for b in centers[i + 1 :]:
            assert max(abs(a[0] - b[0]), abs(a[1] - b[1])) >= 2, "centres too close"
    assert lab.max(initial=-1) < len(centers)
    hm = np.full((h, w), 0.02, np.float32)
    amps = np.linspace(0.95, 0.45, len(centers))
    fg = np.where(lab >= 0, 0.9, 0.1).astype(np.float32)
    off = np.zeros((2, h, w), np.float32)
    yy, xx = np.mgrid[0:h, 0:w]
    for k, (cx, cy) in enumerate(centers):
        hm[cy, cx] = amps[k]
        m = lab == k
        off[0][m] = ((cx - xx) * stride)[m]
        off[1][m] = ((cy - yy) * stride)[m]
    return fg, hm, off


def ring(lab, k, y0, x0, y1, x1, t=1):
    lab[y0 : y1 + 1, x0 : x1 + 1] = k
    lab[y0 + t : y1 + 1 - t, x0 + t : x1 + 1 - t] = -1


def cases():
    out = {}

    def add(name, frames, **kw):
        fg = np.stack([f[0] for f in frames])[:, None]
        hm = np.stack([f[1] for f in frames])[:, None]
        off = np.stack([f[2] for f in frames])
        out[name] = (fg, hm, off, dict(P0, **kw))

    # 1. a ring around a second instance (and some background inside it): the ring fills over both, the inner instance is unchanged
    lab = np.full((24, 31), -1)
    ring(lab, 0, 4, 5, 17, 22, t=2)
    lab[8:13, 10:16] = 1
    lab[20:22, 2:5] = 1  # a smaller fragment of the inner instance, dropped
    ring_frame = paint(lab, [(5, 4), (12, 10)])
    add("ring_around", [ring_frame])

    # 2. three nested rings of three instances; the innermost holds an island of its own label (dropped, then filled over) and a hole
    lab = np.full((40, 44), -1)
    ring(lab, 0, 2, 2, 37, 40, t=2)
    ring(lab, 1, 7, 8, 32, 34, t=2)
    ring(lab, 2, 12, 14, 27, 28, t=2)
    lab[18:21, 19:23] = 2
    lab[19, 20] = -1  # a hole in the island: gone with it
    add("nested_rings", [paint(lab, [(2, 2), (8, 7), (14, 12)])])

    # 3. fragments of equal area: the raster-first one stays; three fragments 6 / 12 / 12: the first of the two largest
    lab = np.full((20, 30), -1)
    lab[2:5, 3:7] = 0
    lab[10:14, 20:23] = 0  # 12 and 12
    lab[2:4, 12:15] = 1
    lab[8:11, 10:14] = 1
    lab[15:19, 3:6] = 1  # 6, 12, 12
    lab[6:8, 22:28] = 2
    lab[6:9, 15:19] = 2  # 12 and 12 starting on the same row: the one further left comes first in raster order
    add("equal_fragments", [paint(lab, [(3, 2), (12, 2), (16, 6)])])

    # 4. fragments that touch only diagonally: a staircase of 2 x 2 blocks, the last one a pixel larger
    lab = np.full((16, 19), -1)
    for i in range(5):
        lab[1 + 2 * i : 3 + 2 * i, 2 + 2 * i : 4 + 2 * i] = 0
    lab[11, 11] = 0  # block 4 gets a fifth pixel
    lab[3, 14], lab[4, 15], lab[5, 14], lab[4, 13] = 1, 1, 1, 1  # four pixels around a free one, touching only diagonally: four fragments, no hole
    add("diagonal", [paint(lab, [(2, 1), (14, 3)])])

    # 5. a cavity open at the image edge (stays) next to one closed only diagonally (filled), on the top, left, bottom and right edges
    lab = np.full((18, 23), -1)
    lab[0:5, 2:8] = 0
    lab[0:4, 4:6] = -1  # open to the top edge
    lab[7:12, 0:6] = 1
    lab[9:10, 0:4] = -1  # open to the left edge
    ring(lab, 2, 1, 11, 6, 17)
    lab[1, 17] = -1  # corner pixel missing: the inside meets the outside only diagonally
    lab[13:18, 9:15] = 3
    lab[15:18, 11:13] = -1  # open to the bottom edge
    lab[9:14, 18:23] = 4
    lab[11, 20:23] = -1  # open to the right edge
    ring(lab, 5, 13, 1, 17, 6)
    lab[13, 1], lab[17, 6] = -1, -1  # two corners missing
    add("cavities", [paint(lab, [(2, 0), (11, 1), (0, 7), (18, 9), (2, 13), (9, 13)])])

    # 6. a serpentine on 40 x 72: one component through every tile of the component pass and across the 64-column word border, a pocket closed at
    # both ends (a hole 68 cells long), open lanes the flood has to walk to their end, and a second instance inside one lane
    lab = np.full((40, 72), -1)
    for i, y in enumerate(range(1, 39, 2)):
        lab[y, 1:71] = 0
        if y + 2 < 39:
            lab[y + 1, 70 if i % 2 == 0 else 1] = 0
    lab[18, 1] = 0  # lane 18 is closed at its right end by the serpentine's turn; close the left end as well
    lab[10, 30:40] = 1
    add("serpentine", [paint(lab, [(1, 1), (30, 10)])])

    # 7. widths that are no multiple of 4 or 64, one row, one column
    lab = np.full((13, 67), -1)
    ring(lab, 0, 1, 1, 11, 65)
    lab[5:8, 30:33] = 0
    ring(lab, 1, 3, 60, 9, 64)
    add("odd_13x67", [paint(lab, [(1, 1), (60, 3)])])
    lab = np.full((1, 41), -1)
    lab[0, 2:5], lab[0, 8:13], lab[0, 20:24], lab[0, 30:34] = 0, 0, 1, 1
    add("one_row", [paint(lab, [(3, 0), (21, 0)])])
    lab = np.full((37, 1), -1)
    lab[2:5, 0], lab[8:13, 0], lab[20:24, 0], lab[30:34, 0] = 0, 0, 1, 1
    add("one_column", [paint(lab, [(0, 3), (0, 21)])])

    # 8. a frame without foreground and one without centres beside a normal one
    fg, hm, off = ring_frame
    no_fg = (np.full_like(fg, 0.1), hm, off)
    no_centre = (fg, np.full_like(hm, 0.02), off)
    add("batch3", [ring_frame, no_fg, no_centre])

    # 9. the distance gate with max_instances top-k, on blobs with punched holes and a far fragment
    def gate_frame(seed):
        fg, hm, off = base.blob_maps(48, 64, 2, [(14, 14), (44, 30), (30, 40)], [0.9, 0.8, 0.7], 8, seed, noise=0.1)
        fg[2:4, 50:62] = 0.9  # strays whose offsets point nowhere near a centre
        off[:, 2:4, 50:62] = 0.0
        fg[13:16, 12:15] = 0.1  # holes
        fg[28:30, 45:47] = 0.1
        fg[30, 38], fg[31, 39] = 0.1, 0.1
        for (x, y) in ((60, 44), (61, 44), (60, 45)):  # a fragment of the second instance far from its blob
            fg[y, x] = 0.9
            off[0, y, x], off[1, y, x] = (44 - x) * 2, (30 - y) * 2
        return fg, hm, off

    add("gate_topk", [gate_frame(30)], distance_gate_alpha=1.6, max_instances=2)

    # 10. more than 127 centres: two-byte labels.  A 3 x 3 ring (hole in the middle) per centre, every third one with a detached pixel
    lab = np.full((96, 97), -1)
    cs = []
    for gy in range(13):
        for gx in range(13):
            k = len(cs)
            x, y = 2 + 7 * gx, 2 + 7 * gy
            ring(lab, k, y, x, y + 2, x + 2)
            if k % 3 == 0:
                lab[y + 4, x + 1] = k
            cs.append((x, y))
    add("many_centres", [paint(lab, cs)])

    # 11. one ring on 640 x 640: its box is beyond the LDS bitmaps of the hole pass
    lab = np.full((640, 640), -1)
    ring(lab, 0, 10, 12, 629, 627, t=3)
    lab[300:310, 300:320] = 1
    lab[305, 310] = -1
    add("big_ring", [paint(lab, [(12, 10), (300, 300)])])
    return out


def run_group_cases(ref_seg):
    out, names = {}, []
    for name, (fg, hm, off, p) in cases().items():
        out[f"group/{name}/fg"], out[f"group/{name}/hm"], out[f"group/{name}/off"] = fg, hm, off
        out[f"group/{name}/params"] = np.array(json.dumps(p))
        for b in range(fg.shape[0]):
            tf, th, to = (torch.from_numpy(a[b : b + 1]) for a in (fg, hm, off))
            peaks, vals = ref_seg.find_center_peaks(th, threshold=p["peak_threshold"], kernel_size=p["center_nms_kernel"])
            all_vals = np.sort(vals.numpy().astype(np.float64))
            if p["max_instances"] is not None and len(peaks) > p["max_instances"]:
                assert np.all(np.diff(all_vals) >= MARGIN), (name, "peak values not distinct")
                vals, keep = torch.topk(vals, p["max_instances"])
                peaks = peaks[keep]
            peaks_np, vals_np = peaks.numpy().astype(np.int32).reshape(-1, 2), vals.numpy().astype(np.float32)
            assert np.all(np.abs(vals_np - p["peak_threshold"]) >= MARGIN), (name, "peak value too close to the threshold")
            base.margins_ok(fg[b, 0], hm[b, 0], off[b], p, peaks_np.astype(np.float64))
            kw = dict(fg_threshold=p["fg_threshold"], peak_threshold=p["peak_threshold"], output_stride=p["output_stride"], max_instances=p["max_instances"],
                      center_nms_kernel=p["center_nms_kernel"], distance_gate_alpha=p["distance_gate_alpha"], distance_gate_iters=p["distance_gate_iters"])
            inst = ref_seg.group_instances_from_offsets(tf, th, to, mask_cleanup=True, **kw)
            raw = ref_seg.group_instances_from_offsets(tf, th, to, mask_cleanup=False, **kw)
            assert len(inst) == len(raw)  # an instance with pixels cannot become empty
            h, w = fg.shape[-2:]
            out[f"group/{name}/{b}/peaks"], out[f"group/{name}/{b}/peak_vals"] = peaks_np, vals_np
            out[f"group/{name}/{b}/masks"] = np.stack([d["mask"] for d in inst]).astype(bool) if inst else np.zeros((0, h, w), bool)
            out[f"group/{name}/{b}/inst_centers"] = np.array([d["center"] for d in inst], dtype=np.float64).reshape(-1, 2)
            out[f"group/{name}/{b}/inst_scores"] = np.array([d["score"] for d in inst], dtype=np.float64)
            changed = sum(int((d["mask"] != r["mask"]).sum()) for d, r in zip(inst, raw))
            overlap = int((np.sum([d["mask"] for d in inst], axis=0) > 1).sum()) if inst else 0
            print(f"group[{name}][{b}]: {len(peaks_np)} centres, {len(inst)} instances, {changed} px changed by cleanup, {overlap} px in more than one mask")
        names.append(name)
    out["group/names"] = np.array(json.dumps(names))
    return out


def run_layer_cases():
    """The area floor is applied to the CLEANED mask: a ring of 64 cells whose fill brings it to 196, and an instance of 12 + 12 cells that falls to 12."""
    from sleap_nn.inference.layers.configs import PostprocessConfig
    from sleap_nn.inference.layers.segmentation import SegmentationLayer
    from sleap_nn.inference.preprocess_info import PreprocInfo

    lab = np.full((24, 32), -1)
    ring(lab, 0, 2, 3, 15, 16)
    lab[18:21, 2:6] = 1
    lab[18:22, 20:23] = 1
    lab[5:9, 26:32] = 2  # reaches into the columns the crop to the valid extent removes
    fg, hm, off = paint(lab, [(3, 2), (24, 5), (2, 18)])
    out, names = {"layer/fg": fg, "layer/hm": hm, "layer/off": off}, []
    orig, proc, eff, iscale, stride = (45, 61), (48, 64), 1.0, 1.0, 2
    for min_area in (0, 60, 300, 800):
        for full in (False, True):
            name = f"a{min_area}/{'full' if full else 'stride'}"
            layer = SegmentationLayer.__new__(SegmentationLayer)
            layer.fg_threshold, layer.min_mask_area, layer.max_instances, layer.full_res_masks, layer.mask_cleanup = 0.5, min_area, None, full, True
            layer.output_stride, layer.postprocess_config = stride, PostprocessConfig(peak_threshold=0.2)
            info = PreprocInfo(original_size=orig, processed_size=proc, eff_scale=torch.tensor([eff], dtype=torch.float32), input_scale=iscale, output_stride=stride)
            raw = {"SegmentationHead": torch.from_numpy(fg)[None, None], "InstanceCenterHead": torch.from_numpy(hm)[None, None], "CenterOffsetHead": torch.from_numpy(off)[None]}
            res = layer.postprocess(raw, info).pred_masks[0]
            layer.mask_cleanup = False
            plain = layer.postprocess(raw, info).pred_masks[0]
            out[f"layer/{name}/n"] = np.array(len(res))
            for i, d in enumerate(res):
                out[f"layer/{name}/{i}/mask"] = np.asarray(d["mask"], dtype=bool)
                out[f"layer/{name}/{i}/meta"] = np.array([d["score"], d["scale"][0], d["scale"][1], d["offset"][0], d["offset"][1]], dtype=np.float64)
            print(f"layer[{name}]: {len(res)} masks with cleanup, {len(plain)} without")
            names.append(name)
    out["layer/names"] = np.array(json.dumps(names))
    out["layer/info"] = np.array(json.dumps([list(orig), list(proc), eff, iscale, stride]))
    return out


def run_dir_case(rh):
    import torch.nn as nn

    from sleap_nn.inference.layers.backends.torch_backend import TorchBackend
    from sleap_nn.inference.layers.configs import PostprocessConfig, PreprocessConfig
    from sleap_nn.inference.layers.segmentation import SegmentationLayer
    from sleap_nn.inference.segmentation import find_center_peaks

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
    m = base.seeded_model(rh, "bottomup_segmentation", 0)
    sd = torch.load(os.path.join(GOLD, "ckpt_dirs", "tiny_bottomup_segmentation", "best.ckpt"), weights_only=False)["state_dict"]
    m.load_state_dict({k[len("model.") :]: v for k, v in sd.items()}, strict=True)

    def layer_for(cleanup):
        return SegmentationLayer(TorchBackend(Fwd(m), device="cpu"), 2, max_stride=base.BB["max_stride"], mask_cleanup=cleanup,
                                 preprocess_config=PreprocessConfig(ensure_grayscale=True), postprocess_config=PostprocessConfig(peak_threshold=P["peak_threshold"]))

    for seed in range(100, 1100):
        frames = base.run_dir_frames(seed)
        x = torch.from_numpy(frames)
        layer = layer_for(True)
        with torch.inference_mode():
            xin, info = layer.preprocess(x)
            raw = layer.backend(xin)
            res = layer.postprocess(raw, info).pred_masks
            plain = layer_for(False).postprocess(raw, info).pred_masks
        fg, hm, off = (raw[k].numpy() for k in ("SegmentationHead", "InstanceCenterHead", "CenterOffsetHead"))
        ok = True
        for b in range(2):
            peaks, vals = find_center_peaks(torch.from_numpy(hm[b : b + 1]), threshold=P["peak_threshold"], kernel_size=3)
            peaks, vals = peaks.numpy().reshape(-1, 2), np.sort(vals.numpy().astype(np.float64))
            if not (2 <= len(peaks) <= 40 and len(res[b]) >= 2 and len(res[b]) == len(plain[b])):
                ok = False
                break
            if (len(vals) > 1 and np.diff(vals).min() < MARGIN) or np.abs(vals - P["peak_threshold"]).min() < MARGIN:
                ok = False
                break
            h0 = hm[b, 0]
            pooled = torch.nn.functional.max_pool2d(torch.from_numpy(hm[b : b + 1]), 3, 1, 1)[0, 0].numpy()
            cand = (h0 >= pooled) & (h0 > P["peak_threshold"])
            if cand.sum() != len(peaks):
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
            if unc.any():
                ok = False
                break
        changed = sum(int((a["mask"] != c["mask"]).sum()) for b in range(2) for a, c in zip(res[b], plain[b])) if ok else 0
        if not ok or changed < 8:  # (a seed on which the cleanup does something)
            continue
        assert not unc.any()
        out = {"rundir/frames": frames, "rundir/params": np.array(json.dumps(dict(P, seed=seed)))}
        for b in range(2):
            out[f"rundir/{b}/n"] = np.array(len(res[b]))
            out[f"rundir/{b}/scores"] = np.array([d["score"] for d in res[b]], dtype=np.float64)
            out[f"rundir/{b}/scales"] = np.array([d["scale"] for d in res[b]], dtype=np.float64).reshape(-1, 2)
            out[f"rundir/{b}/masks"] = np.stack([d["mask"] for d in res[b]])
        print(f"rundir: frames seed {seed}, instances {[len(r) for r in res]}, uncertain set empty, {changed} px changed by cleanup")
        return out
    raise AssertionError("no seed met the run-directory margins")


def main():
    rh = base.install()
    torch.set_num_threads(4)
    import sleap_nn.inference.segmentation as ref_seg

    arrs = {}
    arrs.update(run_group_cases(ref_seg))
    arrs.update(run_layer_cases())
    arrs.update(run_dir_case(rh))
    p = os.path.join(GOLD, "seg_cleanup.npz")
    np.savez_compressed(p, **arrs)
    print(f"wrote {p} ({os.path.getsize(p) / 1024:.0f} KiB, {len(arrs)} arrays)")


if __name__ == "__main__":
    main()
