"""Targets of the identity and top-down model types (sleap_nn_amd/data/targets.py), CPU side: the torch implementations of the contract against the
reference's recorded results (tests/golden/targets_identity.npz, tools/gen_identity_targets_golden.py), and ``TargetGenerator``.

Bounds (the same as the device tests'): confidence maps 2e-6 absolute, the project's rendering bar; class maps ``2e-6 * (1 + I) / threshold``, that error
propagated through ``M / S`` with ``S > threshold``; centroid means 1e-6 absolute, anchors bit for bit."""
import json
import os

import numpy as np
import pytest
import torch

from sleap_nn_amd.data import (TargetGenerator, filter_oob_points, generate_centroids, generate_class_maps, generate_confmaps, make_class_vectors)
from sleap_nn_amd.data.targets import class_map_weights
from tests import _golden as G

CKPT_DIRS = os.path.join(G.GOLDEN_DIR, "ckpt_dirs")


@pytest.fixture(scope="module")
def gold():
    return G.load("targets_identity.npz")


def _names(z, group):
    return json.loads(str(z[f"{group}/names"]))


def class_map_bound(I, threshold):
    return 2e-6 * (1 + I) / threshold


def test_class_maps_match_every_golden_case(gold):
    names = _names(gold, "class_maps")
    assert len(names) == 9
    for name in names:
        p = json.loads(str(gold[f"class_maps/{name}/params"]))
        pts, cls, exp = (gold[f"class_maps/{name}/{k}"] for k in ("points", "class_inds", "expected"))
        out = generate_class_maps(torch.from_numpy(pts), p["img_hw"], torch.from_numpy(cls), p["num_tracks"], class_map_threshold=p["class_map_threshold"],
                                  sigma=p["sigma"], output_stride=p["output_stride"], is_centroids=p["is_centroids"]).numpy()
        assert out.shape == exp.shape and out.dtype == np.float32 and not np.isnan(out).any(), name
        err = float(np.abs(out - exp).max())
        print(f"class maps [{name}]: max error {err:.2e}")
        assert err <= class_map_bound(cls.shape[1], p["class_map_threshold"]), (name, err)


def test_weight_matrix_is_the_references_reshape_not_a_transpose(gold):
    """The fixture's ``weights`` are the reference's ``make_class_vectors`` output under the reshape ``make_class_maps`` applies, restated by the golden tool (the
    reference does not return the matrix), so this compares two statements of the same reshape.  The independent pin of the quirk is
    ``test_class_maps_match_every_golden_case``: the reference's recorded class maps for I != C, which a transposed matrix does not reproduce (checked below)."""
    seen = set()
    for name in _names(gold, "class_maps"):
        p = json.loads(str(gold[f"class_maps/{name}/params"]))
        cls, ref_w = gold[f"class_maps/{name}/class_inds"], gold[f"class_maps/{name}/weights"]
        w = class_map_weights(torch.from_numpy(cls), p["num_tracks"])
        assert w.dtype == torch.float32 and np.array_equal(w.numpy(), ref_w), name
        I, Cn = cls.shape[1], p["num_tracks"]
        transposed = make_class_vectors(torch.from_numpy(cls), Cn).float().transpose(1, 2).numpy()
        if I != Cn and not np.array_equal(ref_w, transposed):
            seen.add(I > Cn)
    assert seen == {True, False}  # I > C and I < C both differ from the transpose in the fixture
    # ... and the recorded class maps really depend on it: with the transpose in its place an I != C case misses its expected output
    from sleap_nn_amd.data.targets import _class_maps_torch

    name = "i5_c3_37x53_s2"
    p = json.loads(str(gold[f"class_maps/{name}/params"]))
    pts, cls = torch.from_numpy(gold[f"class_maps/{name}/points"]), torch.from_numpy(gold[f"class_maps/{name}/class_inds"])
    wrong = _class_maps_torch(pts, make_class_vectors(cls, p["num_tracks"]).float().transpose(1, 2).contiguous(), p["img_hw"], p["class_map_threshold"], p["sigma"], p["output_stride"])
    assert float((wrong - torch.from_numpy(gold[f"class_maps/{name}/expected"])).abs().max()) > 0.1
    # the flattened one-hot rows, cut into C rows of I: instance 0 of class 1 (I = 3, C = 2) weighs (class 0, instance 1)
    assert class_map_weights(torch.tensor([[1, -1, 0]]), 2).tolist() == [[[0.0, 1.0, 0.0], [0.0, 1.0, 0.0]]]


def test_class_map_edge_contracts():
    hw = (12, 20)
    pts = torch.tensor([[[[4.0, 4.0]], [[float("nan"), float("nan")]]]])
    # nothing above the threshold anywhere, S = 0 included: zeros, never NaN
    out = generate_class_maps(torch.full((1, 2, 1, 2), float("nan")), hw, torch.tensor([[0, 1]]), 2)
    assert out.shape == (1, 2, 6, 10) and float(out.abs().max()) == 0.0
    out = generate_class_maps(pts, hw, torch.tensor([[-1, -1]]), 3)  # no class anywhere
    assert float(out.abs().max()) == 0.0
    out = generate_class_maps(pts, hw, torch.tensor([[1, 0]]), 2)
    assert float(out[0, 1, 2, 2]) == 1.0 and float(out[0, 0].max()) == 0.0  # alone at its own grid point: M / S = 1, in its class's channel only
    assert generate_class_maps(torch.zeros((2, 0, 3, 2)), hw, torch.zeros((2, 0), dtype=torch.int32), 2).shape == (2, 2, 6, 10)
    assert generate_class_maps(torch.zeros((0, 2, 3, 2)), hw, torch.zeros((0, 2), dtype=torch.int32), 2).shape == (0, 2, 6, 10)  # an empty batch
    assert generate_confmaps(torch.zeros((0, 3, 2)), hw).shape == (0, 3, 6, 10)
    with pytest.raises(ValueError):
        generate_class_maps(pts, hw, torch.tensor([[0]]), 2)
    with pytest.raises(ValueError):
        generate_class_maps(pts, hw, torch.tensor([[0, 1]]), 2, class_map_threshold=-0.1)


def test_centroids_match_every_golden_case(gold):
    names = _names(gold, "centroids")
    assert names == ["anchor_present", "anchor_nan", "anchor_none", "one_coordinate_nan", "all_nan"]
    for name in names:
        anchor = json.loads(str(gold[f"centroids/{name}/params"]))["anchor_ind"]
        pts, exp = gold[f"centroids/{name}/points"], gold[f"centroids/{name}/expected"]
        out = generate_centroids(torch.from_numpy(pts), anchor_ind=anchor).numpy()
        assert out.shape == exp.shape and np.array_equal(np.isnan(out), np.isnan(exp)), name
        if anchor is not None:
            rows = ~np.isnan(pts[:, anchor]).any(-1)
            assert np.array_equal(out[rows], pts[rows, anchor]), name  # anchors: bit for bit
        err = float(np.nanmax(np.abs(out - exp), initial=0.0))
        print(f"centroids [{name}]: max error {err:.2e}")
        assert err <= 1e-6, (name, err)
    pts = torch.from_numpy(gold["centroids/anchor_nan/points"])
    assert torch.equal(generate_centroids(pts[None, None], anchor_ind=-3)[0, 0], generate_centroids(pts, anchor_ind=2))  # leading axes; Python's negative index
    with pytest.raises(IndexError):
        generate_centroids(pts, anchor_ind=5)


def test_confmaps_filter_and_class_vectors_match_the_goldens(gold):
    for name in _names(gold, "confmaps"):
        p = json.loads(str(gold[f"confmaps/{name}/params"]))
        pts, exp = gold[f"confmaps/{name}/points"], gold[f"confmaps/{name}/expected"]
        out = generate_confmaps(torch.from_numpy(pts), p["img_hw"], sigma=p["sigma"], output_stride=p["output_stride"]).numpy()
        assert out.shape == exp.shape
        np.testing.assert_allclose(out, exp, rtol=0, atol=2e-6)
    p = json.loads(str(gold["filter_oob/params"]))
    out = filter_oob_points(torch.from_numpy(gold["filter_oob/points"]), p["img_height"], p["img_width"]).numpy()
    assert np.array_equal(out, gold["filter_oob/expected"], equal_nan=True)
    assert np.isnan(out[0, 2]).all() and np.isnan(out[0, 3]).all() and not np.isnan(out[0, :2]).any()  # x = width, y = height are out; 0 and size - 1 are in
    out = make_class_vectors(torch.from_numpy(gold["class_vectors/class_inds"]), 3)
    assert out.dtype == torch.int32 and np.array_equal(out.numpy(), gold["class_vectors/expected"])


NAMES = ["a", "b", "c"]
HEADS = {
    "single_instance": {"confmaps": {"part_names": NAMES, "sigma": 2.0, "output_stride": 2}},
    "centroid": {"confmaps": {"anchor_part": "b", "sigma": 3.0, "output_stride": 4}},
    "bottomup": {"confmaps": {"part_names": NAMES, "sigma": 1.5, "output_stride": 2}, "pafs": {"edges": [["a", "b"], ["b", "c"]], "sigma": 10.0, "output_stride": 4}},
    "multi_class_bottomup": {"confmaps": {"part_names": NAMES, "sigma": 1.5, "output_stride": 2}, "class_maps": {"classes": ["x", "y"], "sigma": 2.0, "output_stride": 4}},
    "centered_instance": {"confmaps": {"part_names": NAMES, "anchor_part": "b", "sigma": 1.5, "output_stride": 2}},
    "multi_class_topdown": {"confmaps": {"part_names": NAMES, "anchor_part": "b", "sigma": 1.5, "output_stride": 2},
                            "class_vectors": {"classes": ["x", "y"], "num_fc_layers": 1, "num_fc_units": 8, "output_stride": 8}},
}


def test_target_generator_keys_and_shapes_for_all_six_model_types():
    g = torch.Generator().manual_seed(3)
    hw, B, I = (38, 50), 2, 3
    pts = torch.rand((B, I, 3, 2), generator=g) * torch.tensor([50.0, 38.0])
    pts[0, 2] = float("nan")
    cls = torch.tensor([[0, 1, -1], [1, -1, 0]])
    expect = {
        "single_instance": {"SingleInstanceConfmapsHead": (B, 3, 19, 25)},
        "centroid": {"CentroidConfmapsHead": (B, 1, 10, 13)},
        "bottomup": {"MultiInstanceConfmapsHead": (B, 3, 19, 25), "PartAffinityFieldsHead": (B, 4, 10, 13)},
        "multi_class_bottomup": {"MultiInstanceConfmapsHead": (B, 3, 19, 25), "ClassMapsHead": (B, 2, 10, 13)},
        "centered_instance": {"CenteredInstanceConfmapsHead": (B, 3, 19, 25)},
        "multi_class_topdown": {"CenteredInstanceConfmapsHead": (B, 3, 19, 25), "ClassVectorsHead": (B, 2)},
    }
    for mt, shapes in expect.items():
        tg = TargetGenerator(mt, HEADS[mt], anchor_ind=1)
        one = mt in ("single_instance", "centered_instance", "multi_class_topdown")
        out = tg(pts[:, 0] if one else pts, hw, class_inds=cls[:, 0] if one else cls)
        assert {k: tuple(v.shape) for k, v in out.items()} == shapes, mt
        assert all(v.dtype == torch.float32 and not torch.isnan(v).any() for v in out.values()), mt
    # each head's own sigma and stride; the pieces are the module's functions
    out = TargetGenerator("centroid", HEADS["centroid"], anchor_ind=1)(pts, hw)["CentroidConfmapsHead"]
    cen = generate_centroids(pts, 1)
    assert torch.equal(out, generate_confmaps(cen, hw, sigma=3.0, output_stride=4).amax(dim=1, keepdim=True))
    out = TargetGenerator("multi_class_bottomup", HEADS["multi_class_bottomup"], class_map_threshold=0.3)(pts, hw, cls)["ClassMapsHead"]
    assert torch.equal(out, generate_class_maps(pts, hw, cls, 2, class_map_threshold=0.3, sigma=2.0, output_stride=4))
    crop = pts[:, 0].clone()
    crop[1, 0] = torch.tensor([50.0, 10.0])  # x = width: outside the crop, so its map is empty
    out = TargetGenerator("multi_class_topdown", HEADS["multi_class_topdown"])(crop, hw, torch.tensor([1, -1]))
    assert float(out["CenteredInstanceConfmapsHead"][1, 0].max()) == 0.0 and float(out["CenteredInstanceConfmapsHead"][1, 1].max()) > 0.5
    assert out["ClassVectorsHead"].tolist() == [[0.0, 1.0], [0.0, 0.0]]
    with pytest.raises(ValueError):
        TargetGenerator("multi_class_bottomup", HEADS["multi_class_bottomup"])(pts, hw)


def test_target_generator_bottomup_cpu_targets_match_the_reference_fixture():
    """The CPU form of the bottom-up targets (the device kernels' contract in torch) against tests/golden/targets.npz, at the GPU test's tolerances."""
    z = G.load("targets.npz")
    meta = json.loads(str(z["meta_json"]))
    pts = torch.from_numpy(z["points"])
    names = [str(i) for i in range(pts.shape[2])]
    for (cs, csig), (ps, psig) in zip(meta["confmaps"], meta["pafs"]):
        heads = {"confmaps": {"part_names": names, "sigma": csig, "output_stride": cs},
                 "pafs": {"edges": [[names[a], names[b]] for a, b in meta["edges"]], "sigma": psig, "output_stride": ps}}
        out = TargetGenerator("bottomup", heads)(pts, meta["hw"])
        np.testing.assert_allclose(out["MultiInstanceConfmapsHead"].numpy(), z[f"confmaps_s{cs}"], rtol=0, atol=2e-6)
        np.testing.assert_allclose(out["PartAffinityFieldsHead"].numpy(), z[f"pafs_s{ps}"], rtol=0, atol=5e-6)


def test_from_training_config_on_the_committed_run_directories():
    tg = TargetGenerator.from_training_config(os.path.join(CKPT_DIRS, "minimal_instance_bottomup", "training_config.yaml"))
    assert tg.model_type == "bottomup" and tg.edge_inds == [(0, 1)]
    h = tg.heads
    assert (h["MultiInstanceConfmapsHead"].sigma, h["MultiInstanceConfmapsHead"].output_stride) == (1.5, 2)
    assert (h["PartAffinityFieldsHead"].sigma, h["PartAffinityFieldsHead"].output_stride) == (50.0, 4)
    out = tg(torch.tensor([[[[10.0, 12.0], [30.0, 20.0]]]]), (48, 64))
    assert {k: tuple(v.shape) for k, v in out.items()} == {"MultiInstanceConfmapsHead": (1, 2, 24, 32), "PartAffinityFieldsHead": (1, 2, 12, 16)}
    tg = TargetGenerator.from_training_config(os.path.join(CKPT_DIRS, "minimal_instance_single_instance"))  # a run directory
    assert tg.model_type == "single_instance" and tg.anchor_ind is None
    assert tuple(tg(torch.tensor([[[10.0, 12.0], [30.0, 20.0]]]), (48, 64))["SingleInstanceConfmapsHead"].shape) == (1, 2, 12, 16)
    # anchor_part goes through the skeleton's node names
    import yaml

    with open(os.path.join(CKPT_DIRS, "minimal_instance_single_instance", "training_config.yaml")) as f:
        cfg = yaml.safe_load(f)
    cfg["model_config"]["head_configs"] = {"single_instance": None, "centroid": {"confmaps": {"anchor_part": "B", "sigma": 2.0, "output_stride": 2}}}
    tg = TargetGenerator.from_training_config(cfg)
    assert tg.model_type == "centroid" and tg.anchor_ind == 1
    cfg["model_config"]["head_configs"]["centroid"]["confmaps"]["anchor_part"] = "nose"
    with pytest.raises(ValueError):
        TargetGenerator.from_training_config(cfg)


def test_segmentation_model_types_are_refused():
    for name in ("tiny_bottomup_segmentation", "tiny_semantic_segmentation"):
        with pytest.raises(NotImplementedError):
            TargetGenerator.from_training_config(os.path.join(CKPT_DIRS, name))
    for mt in ("bottomup_segmentation", "semantic_segmentation", "centered_instance_segmentation"):
        with pytest.raises(NotImplementedError):
            TargetGenerator(mt, {"segmentation": {"output_stride": 2}})
