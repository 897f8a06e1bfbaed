"""Generate ``tests/golden/targets_identity.npz`` from the reference's own code (through ``oracle.ref_harness``, where the reference tree is available):
the targets of the identity and top-down model types -- ``generate_class_maps``, ``generate_centroids``, ``generate_confmaps``, ``filter_oob_points``,
``make_class_vectors`` -- on small inputs.  Per case: the inputs, the parameters as JSON, and what the reference returns.

The reference works on one frame at a time; a batched case is its frames one after the other, each with ``num_instances = I`` (instances beyond a
frame's count are all-NaN rows with class -1, which is how the batched functions of ``sleap_nn_amd.data.targets`` take them).

Class maps are discontinuous where an instance's map crosses ``class_map_threshold``.  No recorded decision may hang on the last bits: the tool asserts
that no (pixel, instance) pair has ``|M_i - threshold| < 1e-4`` (fifty times the 2e-6 rendering error) and replaces a seed that misses, so the tests
exclude nothing.

    python tools/gen_identity_targets_golden.py
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GOLD = os.path.join(ROOT, "tests", "golden")
MARGIN = 1e-4
NAN = float("nan")


def random_points(g, B, I, N, hw, nan_frac=0.15):
    """(B, I, N, 2): each instance a cluster of nodes around a centre somewhere in (and a little beyond) the image."""
    H, W = hw
    centre = g.uniform([-2, -2], [W + 2, H + 2], size=(B, I, 1, 2))
    pts = centre + g.normal(0, max(2.0, min(H, W) / 8), size=(B, I, N, 2))
    pts[g.random((B, I, N)) < nan_frac] = NAN
    return pts.astype(np.float32)


def class_map_cases(seed):
    """name -> (points (B, I, N, 2) or (B, I, 2), class_inds (B, I), params)."""
    g = np.random.default_rng(seed)
    P = dict(class_map_threshold=0.2, sigma=1.5, output_stride=2, is_centroids=False)
    cases = {}

    def add(name, pts, cls, hw, C, **kw):
        cases[name] = (pts, np.asarray(cls, dtype=np.int32), dict(P, img_hw=list(hw), num_tracks=C, **kw))

    # neither size a multiple of the stride or of a wave; I != C both ways, I = C, I = 1
    add("i5_c3_37x53_s2", random_points(g, 1, 5, 4, (37, 53)), [[0, 2, 1, 1, 0]], (37, 53), 3)
    add("i3_c5_67x41_s4", random_points(g, 1, 3, 6, (67, 41)), [[4, 0, 2]], (67, 41), 5, output_stride=4, sigma=2.0)
    add("i4_c4_37x53_s2", random_points(g, 1, 4, 3, (37, 53)), [[3, 1, 0, 2]], (37, 53), 4)
    add("i1_c2_37x53_s2", random_points(g, 1, 1, 5, (37, 53), nan_frac=0.0), [[1]], (37, 53), 2)
    add("one_row_1x41", np.array([[[[6.0, 0.0], [11.0, 0.3]], [[30.0, 0.0], [NAN, NAN]]]], np.float32), [[0, 1]], (1, 41), 2)
    # a class index of -1, an all-NaN instance, a node with ONE NaN coordinate
    pts = random_points(g, 1, 4, 4, (37, 53), nan_frac=0.0)
    pts[0, 2] = NAN
    pts[0, 1, 1, 0] = NAN
    add("no_class_allnan_halfnan", pts, [[1, -1, 0, 2]], (37, 53), 3)
    # two instances closer than one sigma (sigma * stride = 3 px): both above the threshold around them, so the normalisation decides
    close = np.array([[[[20.0, 15.0], [26.0, 18.0]], [[21.5, 16.0], [27.0, 19.5]], [[44.0, 30.0], [40.0, 25.0]]]], np.float32)
    add("two_close", close, [[0, 1, 1]], (37, 53), 2)
    # centroids: N = 1
    add("centroids_i5_c3", random_points(g, 1, 5, 1, (37, 53), nan_frac=0.0)[:, :, 0], [[2, 0, 1, -1, 0]], (37, 53), 3, is_centroids=True)
    # a batch of 3 whose middle frame has no instances (all-NaN rows, class -1); the last frame has two
    pts = random_points(g, 3, 3, 4, (37, 53))
    pts[1] = NAN
    pts[2, 2] = NAN
    add("batch3_empty_middle", pts, [[0, 1, 2], [-1, -1, -1], [2, 0, -1]], (37, 53), 4)
    return cases


def instance_maps(pts, hw, sigma, stride):
    """float64 per-instance maps (I, h, w) of one frame's (I, N, 2) points: the margin check's own arithmetic."""
    xv, yv = np.arange(0, hw[1], stride, dtype=np.float64), np.arange(0, hw[0], stride, dtype=np.float64)
    p = pts.astype(np.float64)
    d2 = (xv[None, None, None, :] - p[..., 0, None, None]) ** 2 + (yv[None, None, :, None] - p[..., 1, None, None]) ** 2
    m = np.nan_to_num(np.exp(-d2 / (2 * (sigma * stride) ** 2)))
    return m.max(axis=1)


def run_class_maps(ref_identity):
    for seed in range(200, 260):
        out, names, ok = {}, [], True
        for name, (pts, cls, p) in class_map_cases(seed).items():
            pts4 = pts[:, :, None] if p["is_centroids"] else pts
            B, I = cls.shape
            frames = []
            for b in range(B):
                m = instance_maps(pts4[b], p["img_hw"], p["sigma"], p["output_stride"])
                if np.abs(m - p["class_map_threshold"]).min() < MARGIN:
                    ok = False
                    break
                frames.append(ref_identity.generate_class_maps(torch.from_numpy(pts[b : b + 1]), tuple(p["img_hw"]), I, torch.from_numpy(cls[b]), p["num_tracks"],
                                                               class_map_threshold=p["class_map_threshold"], sigma=p["sigma"], output_stride=p["output_stride"],
                                                               is_centroids=p["is_centroids"])[0].numpy())
            if not ok:
                break
            exp = np.stack(frames)
            assert exp.dtype == np.float32 and not np.isnan(exp).any(), name
            out[f"class_maps/{name}/points"], out[f"class_maps/{name}/class_inds"] = pts, cls
            out[f"class_maps/{name}/params"], out[f"class_maps/{name}/expected"] = np.array(json.dumps(p)), exp
            # The reference's make_class_vectors output under the same torch.reshape call make_class_maps applies to it (identity.py:66-69), restated HERE: the
            # reference does not return that matrix.  What pins the quirk independently is `expected` above for I != C, which only that matrix reproduces.
            out[f"class_maps/{name}/weights"] = np.stack([ref_identity.make_class_vectors(torch.from_numpy(cls[b]), p["num_tracks"]).to(torch.float32)
                                                          .reshape(p["num_tracks"], I).numpy() for b in range(B)])
            names.append(name)
            print(f"class_maps[{name}]: {exp.shape}, non-zero {float((exp > 0).mean()):.3f}, max {float(exp.max()):.3f}")
        if ok:
            out["class_maps/names"] = np.array(json.dumps(names))
            out["class_maps/seed"] = np.array(seed)
            return out
        print(f"seed {seed}: a map value within {MARGIN} of the threshold; next seed")
    raise AssertionError("no seed met the threshold margin")


def run_centroids(ref_centroids):
    g = np.random.default_rng(7)
    base = g.uniform(0, 300, size=(3, 5, 2)).astype(np.float32)
    cases = {}
    cases["anchor_present"] = (base.copy(), 2)
    a = base.copy()
    a[1, 2] = NAN  # the anchor of instance 1 is missing: its mean; the others keep their anchor
    a[2, 2, 1] = NAN  # ... of instance 2 has one coordinate: also the mean
    cases["anchor_nan"] = (a, 2)
    cases["anchor_none"] = (base.copy(), None)
    a = base.copy()
    a[0, 1, 0] = NAN
    a[1, 3, 1] = NAN
    a[1, 0, 1] = NAN
    cases["one_coordinate_nan"] = (a, None)
    a = base.copy()
    a[1] = NAN
    cases["all_nan"] = (a, 0)
    out, names = {}, []
    for name, (pts, anchor) in cases.items():
        exp = ref_centroids.generate_centroids(torch.from_numpy(pts[None]), anchor_ind=anchor)[0].numpy()
        out[f"centroids/{name}/points"], out[f"centroids/{name}/expected"] = pts, exp
        out[f"centroids/{name}/params"] = np.array(json.dumps({"anchor_ind": anchor}))
        names.append(name)
        print(f"centroids[{name}]: {exp.tolist()}")
    out["centroids/names"] = np.array(json.dumps(names))
    return out


def run_confmaps(ref_confmaps):
    g = np.random.default_rng(11)
    out = {}
    p3 = random_points(g, 2, 1, 5, (37, 53))[:, 0]
    p4 = random_points(g, 2, 3, 4, (67, 41))
    for name, pts, p in (("3d", p3, dict(img_hw=[37, 53], sigma=1.5, output_stride=2)), ("4d", p4, dict(img_hw=[67, 41], sigma=2.0, output_stride=4))):
        exp = ref_confmaps.generate_confmaps(torch.from_numpy(pts), tuple(p["img_hw"]), sigma=p["sigma"], output_stride=p["output_stride"]).numpy()
        out[f"confmaps/{name}/points"], out[f"confmaps/{name}/expected"], out[f"confmaps/{name}/params"] = pts, exp, np.array(json.dumps(p))
        print(f"confmaps[{name}]: {pts.shape} -> {exp.shape}")
    out["confmaps/names"] = np.array(json.dumps(["3d", "4d"]))
    return out


def run_filter_oob(ref_providers):
    h, w = 37, 53
    pts = np.array([[[0.0, 0.0], [52.0, 36.0], [53.0, 10.0], [10.0, 37.0], [52.999, 36.999], [-0.001, 5.0], [5.0, -1.0], [NAN, 5.0], [5.0, NAN], [NAN, 40.0], [60.0, NAN],
                     [20.5, 11.25]]], np.float32)
    exp = ref_providers.filter_oob_points(torch.from_numpy(pts), h, w).numpy()
    print(f"filter_oob: kept {int((~np.isnan(exp).any(-1)).sum())} of {pts.shape[1]}")
    return {"filter_oob/points": pts, "filter_oob/expected": exp, "filter_oob/params": np.array(json.dumps({"img_height": h, "img_width": w}))}


def run_class_vectors(ref_identity):
    cls = np.array([2, -1, 0, 1, -1], np.int32)
    return {"class_vectors/class_inds": cls, "class_vectors/expected": ref_identity.make_class_vectors(torch.from_numpy(cls), 3).numpy(),
            "class_vectors/params": np.array(json.dumps({"n_classes": 3}))}


def main():
    from oracle import ref_harness as rh

    rh.install()
    torch.set_num_threads(4)
    import sleap_nn.data.confidence_maps as ref_confmaps
    import sleap_nn.data.identity as ref_identity
    import sleap_nn.data.instance_centroids as ref_centroids
    import sleap_nn.data.providers as ref_providers

    arrs = {}
    arrs.update(run_class_maps(ref_identity))
    arrs.update(run_centroids(ref_centroids))
    arrs.update(run_confmaps(ref_confmaps))
    arrs.update(run_filter_oob(ref_providers))
    arrs.update(run_class_vectors(ref_identity))
    p = os.path.join(GOLD, "targets_identity.npz")
    np.savez_compressed(p, **arrs)
    print(f"wrote {p} ({os.path.getsize(p) / 1024:.0f} KiB, {len(arrs)} arrays)")


if __name__ == "__main__":
    main()
