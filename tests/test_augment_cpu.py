"""Training augmentation, host side: the per-sample draws replayed against the reference's own functions
(tests/golden/augment_draws.npz, tools/gen_augment_golden.py), config loading from run directories, the C ABI's
parameter record.  No GPU needed."""
import ctypes
import inspect
import json
import os

import numpy as np
import pytest

from sleap_nn_amd import _lib as L
from sleap_nn_amd.data import augmentation as A
from tests import _golden as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RUN_DIRS = [os.path.join(ROOT, "tests", "golden", "ckpt_dirs", d) for d in ("minimal_instance_bottomup", "minimal_instance_single_instance")]


def _kw_defaults(fn):
    return {k: p.default for k, p in inspect.signature(fn).parameters.items() if p.default is not inspect.Parameter.empty and k not in ("rng", "symmetric_inds")}


def _fixture_cases():
    z = G.load("augment_draws.npz")
    cfgs = json.loads(str(z["configs_json"]))
    return [(name, int(seed)) for name in cfgs for seed in z["seeds"]]


@pytest.mark.parametrize("name,seed", _fixture_cases())
def test_draws_replay_the_reference(name, seed):
    """Matrices, flips, erase rectangles and fills, contrast / brightness factors, the NumPy state after the batch, and
    the keypoints mapped on the host, for every fixture config and seed."""
    z = G.load("augment_draws.npz")
    c = json.loads(str(z["configs_json"]))[name]
    icfg = {**_kw_defaults(A.apply_intensity_augmentation), **c["intensity"]}
    gcfg = {**_kw_defaults(A.apply_geometric_augmentation), **c["geometric"]}
    sym = [tuple(p) for p in c["symmetric"]]
    h, w = c["hw"]
    rng = np.random.RandomState(seed)
    aug = A.Augmenter(icfg, gcfg, sym, rng=rng)
    n = int(z["samples"])
    draws, noise_seed = aug.draw(n, (h, w), c["channels"])
    p = f"{name}/s{seed}/"
    assert noise_seed == 0
    st = rng.get_state()
    assert np.array_equal(st[1], z[p + "state_key"]) and st[2] == int(z[p + "state_pos"])
    for i, d in enumerate(draws):
        assert d.warp == bool(z[p + "warp"][i]), i
        assert d.flip == bool(z[p + "flip"][i]), i
        m = z[p + "matrix"][i]
        assert np.allclose(d.matrix, m, rtol=1e-6, atol=1e-6 * float(np.abs(m).max())), (i, d.matrix, m)
        er = tuple(int(v) for v in z[p + "erase"][i])
        assert (d.erase if d.erase is not None else (-1, -1, -1, -1)) == er, i
        if d.erase is not None:
            assert list(d.fill) == [int(v) for v in z[p + "fill"][i][: c["channels"]]]
        for got, key in ((d.contrast, "contrast"), (d.brightness, "brightness")):
            want = float(z[p + key][i])
            assert (got is None and np.isnan(want)) or got == want, (i, key, got, want)
        # keypoints: flip ((W-1) - x, pairs swapped in order), then the skia matrix
        kp = z[p + "keypoints"][i].copy()
        if d.flip:
            kp[..., 0] = (w - 1) - kp[..., 0]
            for a, b in sym:
                kp[..., [a, b], :] = kp[..., [b, a], :]
        if d.warp:
            kp = A.map_points(d.matrix, kp)
        want = z[p + "mapped"][i]
        assert np.array_equal(np.isnan(kp), np.isnan(want))
        assert np.allclose(kp, want, atol=1e-4, equal_nan=True)


def test_function_keyword_defaults_are_the_reference_ones_and_config_defaults_are_attrs():
    z = G.load("augment_draws.npz")
    assert A.INTENSITY_DEFAULTS == json.loads(str(z["intensity_defaults_json"]))
    assert A.GEOMETRIC_DEFAULTS == json.loads(str(z["geometric_defaults_json"]))
    g = _kw_defaults(A.apply_geometric_augmentation)
    # sleap_nn/data/augmentation.py keyword defaults (independent probabilities off, 2 % translation)
    assert g["rotation_p"] is None and g["scale_p"] is None and g["translate_p"] is None and g["translate_width"] == 0.02 and g["affine_p"] == 0.0
    assert _kw_defaults(A.apply_intensity_augmentation) == A.INTENSITY_DEFAULTS


def test_intensity_lut_formula_matches_reference_output():
    """The reference's contrast / brightness LUTs (float32, truncating casts) restated in NumPy give its own output."""
    z = G.load("augment_draws.npz")
    for i in range(4):
        x, y = z[f"intensity/{i}/input"], z[f"intensity/{i}/output"]
        c, b = float(z[f"intensity/{i}/contrast"]), float(z[f"intensity/{i}/brightness"])
        v = np.arange(256, dtype=np.float32)
        lut = np.clip((v - np.float32(127.5)) * np.float32(c) + np.float32(127.5), 0, 255).astype(np.uint8)
        if not np.isnan(b):
            lut = np.clip(lut.astype(np.float32) * np.float32(b), 0, 255).astype(np.uint8)
        assert np.array_equal(lut[x], y), i


@pytest.mark.parametrize("run_dir", RUN_DIRS)
def test_config_from_run_dir_takes_attrs_defaults(run_dir):
    import yaml

    aug = A.Augmenter.from_run_dir(run_dir)
    y = yaml.safe_load(open(os.path.join(run_dir, "training_config.yaml")))["data_config"]
    assert y["use_augmentations_train"] is True
    geo = y["augmentation_config"]["geometric"]
    assert "rotation_p" not in geo and "scale_p" not in geo and "mixup_p" in geo
    # what OmegaConf.structured builds: attrs defaults under the YAML's keys -> independent rotation and scale, always on
    assert aug.geometric == {**A.GEOMETRIC_DEFAULTS, **geo}
    assert aug.geometric["rotation_p"] == 1.0 and aug.geometric["scale_p"] == 1.0 and aug.geometric["translate_p"] is None
    assert (aug.geometric["rotation_min"], aug.geometric["rotation_max"]) == (-180.0, 180.0)
    assert aug.intensity == {**A.INTENSITY_DEFAULTS, **y["augmentation_config"]["intensity"]}
    assert aug.symmetric_inds == []
    draws, seed = aug.draw(8, (64, 64))
    assert all(d.warp for d in draws) and not any(d.flip or d.erase for d in draws) and seed == 0


def test_config_switches_symmetries_and_errors():
    import warnings

    base = {"data_config": {"use_augmentations_train": False, "augmentation_config": {"geometric": {"rotation_p": 1.0}},
                            "skeletons": [{"nodes": [{"name": "a"}, {"name": "l"}, {"name": "r"}], "symmetries": [[{"name": "r"}, {"name": "l"}]]}]}}
    off = A.Augmenter.from_training_config(base)
    assert off.intensity is None and off.geometric is None and off.symmetric_inds == [(2, 1)]
    st = np.random.get_state()[1].copy()
    draws, seed = off.draw(3, (16, 16))
    assert seed == 0 and not any(d.warp or d.flip or d.erase or d.contrast or d.brightness for d in draws)
    assert np.array_equal(np.random.get_state()[1], st)  # nothing drawn
    on = dict(base["data_config"], use_augmentations_train=True, augmentation_config={"intensity": None, "geometric": {"flip_p": 0.5, "mixup_p": 0.3}})
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        a = A.Augmenter.from_training_config({"data_config": on})  # symmetries present: no warning
    assert a.intensity is None and a.geometric["flip_p"] == 0.5 and a.geometric["mixup_p"] == 0.3
    no_sym = dict(on, skeletons=[{"nodes": [{"name": "a"}], "symmetries": []}])
    with pytest.warns(UserWarning, match="no symmetries"):
        A.Augmenter.from_training_config({"data_config": no_sym})
    with pytest.raises(ValueError, match="unknown geometric"):
        A.Augmenter(None, {"rotate": 3})
    with pytest.raises(ValueError, match="channels"):
        A.Augmenter(None, {}).draw(1, (8, 8), channels=2)


def test_parameter_record_matches_the_library():
    assert L.lib().ph_aug_sample_size() == ctypes.sizeof(L.AugSample) == 160


def test_packed_inverse_and_frame_edges():
    """minv undoes the skia matrix (and the flip, as x -> W - x); the four half-planes hold the mapped frame."""
    h, w = 30, 50
    d = A.SampleDraw(flip=True, warp=True, matrix=A._concat(A._rotate(33.0, w / 2, h / 2), A._scale(0.7, 0.7, w / 2, h / 2)))
    rec = A._pack([d], h, w, None, 0)[0]
    m = np.array(list(rec.m), np.float64)
    inv = np.array(list(rec.minv), np.float64)
    for x, y in ((0.0, 0.0), (12.5, 7.25), (49.0, 29.0)):
        X, Y = m[0] * x + m[1] * y + m[2], m[3] * x + m[4] * y + m[5]
        assert np.allclose((inv[0] * X + inv[1] * Y + inv[2], inv[3] * X + inv[4] * Y + inv[5]), (w - x, y), atol=1e-4)
    e = np.array(list(rec.edge), np.float64).reshape(4, 3)
    inside = lambda x, y: (e[:, 0] * x + e[:, 1] * y + e[:, 2] >= -1e-4).all()  # noqa: E731
    for x, y in ((0, 0), (w, 0), (w, h), (0, h), (w / 2, h / 2)):
        assert inside(m[0] * x + m[1] * y + m[2], m[3] * x + m[4] * y + m[5])
    assert not inside(m[0] * -1 + m[2], m[3] * -1 + m[5])
    assert rec.flags == L.AUG_FLIP | L.AUG_WARP
