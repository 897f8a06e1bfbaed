"""Generate tests/golden/augment_draws.npz from the reference's own augmentation functions.

Runs ``apply_intensity_augmentation_skia`` and ``apply_geometric_augmentation_skia`` of the reference
(``sleap_nn/data/skia_augmentation.py``, imported through ``oracle.ref_harness``) per sample, the way its dataset calls
them (``data/custom_datasets.py:1101-1117``), under fixed global NumPy seeds with noise off, and records what they drew:
the skia matrices handed to the canvas, the flip decisions, the erase rectangles and fills, the contrast / brightness
factors, the mapped keypoints and the NumPy state after each batch.  It also records the attrs defaults of
``IntensityConfig`` / ``GeometricConfig`` and full image outputs of the (pure NumPy) intensity function for contrast and
brightness on small frames.

skia is not installed where this runs, so a small NumPy stand-in for ``skia.Matrix`` / ``skia.Point`` is registered
below (float32 entries, as SkScalar; concatenation in double then rounded, as SkMatrix::setConcat), with ``Image`` /
``Surface`` / ``Canvas`` stubs that only record the matrix.  The matrix arithmetic in the fixture therefore rests on this
stand-in's restatement of skia; the call order and every random draw are the reference's own.  The warp's pixels cannot be
pinned to skia without skia: their contract is the formula in DESIGN.md section 9, restated by tests/test_gpu_augment.py.

    python tools/gen_augment_golden.py [out.npz]
"""
from __future__ import annotations

import importlib
import json
import linecache
import math
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

F32 = np.float32


# ---------------------------------------------------------------------------------------------------------------------
# skia stand-in
# ---------------------------------------------------------------------------------------------------------------------
class Point:
    def __init__(self, x, y):
        self._x, self._y = F32(x), F32(y)

    def x(self):
        return float(self._x)

    def y(self):
        return float(self._y)


class Matrix:
    """SkMatrix, affine part: [scaleX, skewX, transX, skewY, scaleY, transY]."""

    def __init__(self):
        self.v = np.array([1, 0, 0, 0, 1, 0], dtype=F32)

    def setRotate(self, degrees, px=0.0, py=0.0):
        rad = F32(degrees) * F32(math.pi / 180.0)
        s, c = np.sin(rad, dtype=F32), np.cos(rad, dtype=F32)
        s = F32(0) if abs(float(s)) <= 1.0 / 4096 else s
        c = F32(0) if abs(float(c)) <= 1.0 / 4096 else c
        px, py = F32(px), F32(py)
        self.v = np.array([c, -s, s * py + (F32(1) - c) * px, s, c, -s * px + (F32(1) - c) * py], dtype=F32)
        return self

    def setScale(self, sx, sy, px=0.0, py=0.0):
        sx, sy, px, py = F32(sx), F32(sy), F32(px), F32(py)
        if sx == 1 and sy == 1:
            self.v = np.array([1, 0, 0, 0, 1, 0], dtype=F32)
        else:
            self.v = np.array([sx, 0, px - sx * px, 0, sy, py - sy * py], dtype=F32)
        return self

    def setTranslate(self, dx, dy):
        self.v = np.array([1, 0, F32(dx), 0, 1, F32(dy)], dtype=F32)
        return self

    def preConcat(self, other):
        a, b = self.v, other.v

        def mam(p, q, r, s):
            return F32(float(p) * float(q) + float(r) * float(s))

        self.v = np.array([mam(a[0], b[0], a[1], b[3]), mam(a[0], b[1], a[1], b[4]), mam(a[0], b[2], a[1], b[5]) + a[2],
                           mam(a[3], b[0], a[4], b[3]), mam(a[3], b[1], a[4], b[4]), mam(a[3], b[2], a[4], b[5]) + a[5]], dtype=F32)
        return self

    def preScale(self, sx, sy, px=0.0, py=0.0):
        if F32(sx) == 1 and F32(sy) == 1:
            return self
        return self.preConcat(Matrix().setScale(sx, sy, px, py))

    def preTranslate(self, dx, dy):
        dx, dy = F32(dx), F32(dy)
        v = self.v.copy()
        if v[0] == 1 and v[1] == 0 and v[3] == 0 and v[4] == 1:
            v[2] += dx
            v[5] += dy
        else:
            v[2] = v[2] + (v[0] * dx + v[1] * dy)
            v[5] = v[5] + (v[3] * dx + v[4] * dy)
        self.v = v
        return self

    def mapPoints(self, pts):
        v = self.v
        return [Point((p._x * v[0] + p._y * v[1]) + v[2], (p._x * v[3] + p._y * v[4]) + v[5]) for p in pts]


RECORD = {"matrix": None}


class _Canvas:
    def clear(self, *a):
        pass

    def setMatrix(self, m):
        RECORD["matrix"] = m.v.copy()

    def drawImage(self, *a, **k):
        pass


class _Surface:
    def __init__(self, arr, colorType=None):
        self.arr = arr

    def getCanvas(self):
        return _Canvas()

    def flushAndSubmit(self):
        pass


class _Any:
    def __init__(self, *a, **k):
        pass

    def __getattr__(self, k):
        return lambda *a, **kw: None


def _skia_module():
    m = types.ModuleType("skia")
    m.Matrix, m.Point, m.Surface = Matrix, Point, _Surface
    m.Image = types.SimpleNamespace(fromarray=lambda *a, **k: None)
    m.ColorType = types.SimpleNamespace(kRGBA_8888_ColorType=0)
    m.FilterMode = types.SimpleNamespace(kLinear=0, kNearest=1)
    m.Color4f = m.Paint = m.SamplingOptions = _Any
    return m


# ---------------------------------------------------------------------------------------------------------------------
# draw log: every np.random call of the reference module, tagged with its source line
# ---------------------------------------------------------------------------------------------------------------------
class _RandomProxy:
    def __init__(self, log):
        self._log = log

    def __getattr__(self, name):
        fn = getattr(np.random, name)

        def wrapped(*a, **k):
            r = fn(*a, **k)
            fr = sys._getframe(1)
            self._log.append((name, linecache.getline(fr.f_code.co_filename, fr.f_lineno).strip(), r))
            return r

        return wrapped


class _NpProxy:
    def __init__(self, log):
        self.random = _RandomProxy(log)

    def __getattr__(self, k):
        return getattr(np, k)


def load_reference():
    sys.modules["skia"] = _skia_module()
    from oracle import ref_harness as R

    R.install()
    sk = importlib.import_module("sleap_nn.data.skia_augmentation")
    cfg_pkg = types.ModuleType("sleap_nn.config")
    cfg_pkg.__path__ = [os.path.join(R.REFERENCE_ROOT, "sleap_nn", "config")]
    sys.modules.setdefault("sleap_nn.config", cfg_pkg)
    dc = importlib.import_module("sleap_nn.config.data_config")
    return sk, dc


INT_OFF = dict(uniform_noise_p=0.0, gaussian_noise_p=0.0)
ATTR_GEO = {"rotation_min": -180.0, "rotation_max": 180.0, "rotation_p": 1.0, "scale_min": 0.9, "scale_max": 1.1, "scale_p": 1.0, "translate_width": 0.0,
            "translate_height": 0.0, "translate_p": None, "affine_p": 0.0, "erase_scale_min": 0.0001, "erase_scale_max": 0.01, "erase_ratio_min": 1.0,
            "erase_ratio_max": 1.0, "erase_p": 0.0, "mixup_lambda_min": 0.01, "mixup_lambda_max": 0.05, "mixup_p": 0.0, "flip_p": 0.0}
CONFIGS = {
    # name: (channels, (h, w), intensity kwargs, geometric kwargs, symmetric pairs)
    "independent": (1, (48, 64), dict(INT_OFF, contrast_min=0.5, contrast_max=2.0, contrast_p=0.6, brightness_min=0.5, brightness_max=1.5, brightness_p=0.5),
                    dict(rotation_min=-180.0, rotation_max=180.0, rotation_p=1.0, scale_min=0.5, scale_max=1.5, scale_p=0.5, translate_width=0.1,
                         translate_height=0.05, translate_p=0.7), []),
    "bundled": (3, (40, 56), dict(INT_OFF, contrast_p=0.5), dict(rotation_min=-30.0, rotation_max=30.0, rotation_p=None, scale_min=0.8, scale_max=1.2, scale_p=None,
                                                                translate_width=0.1, translate_height=0.1, translate_p=None, affine_p=0.8), []),
    "flip": (1, (48, 64), dict(INT_OFF), dict(rotation_min=-90.0, rotation_max=90.0, rotation_p=0.5, scale_p=None, translate_p=None, flip_p=0.5), [(0, 1), (2, 3)]),
    "erase": (3, (40, 56), dict(INT_OFF, brightness_p=0.3), dict(rotation_p=0.0, scale_p=None, translate_p=None, erase_p=0.7, erase_scale_min=0.01, erase_scale_max=0.2,
                                                               erase_ratio_min=0.5, erase_ratio_max=2.0), []),
    "fixture_yaml": (1, (48, 64), dict(INT_OFF, contrast_min=0.5, contrast_max=2.0, brightness_min=0.0, brightness_max=2.0), dict(ATTR_GEO), []),
    "everything": (3, (40, 56), dict(INT_OFF, contrast_p=0.5, brightness_p=0.5),
                   dict(rotation_min=-180.0, rotation_max=180.0, rotation_p=0.8, scale_min=0.25, scale_max=1.5, scale_p=0.8, translate_width=0.2, translate_height=0.2,
                        translate_p=0.5, erase_p=0.5, erase_scale_min=0.001, erase_scale_max=0.05, flip_p=0.5), [(1, 2)]),
}
SEEDS = (0, 1, 7)
SAMPLES = 6


def main(out_path):
    import torch

    sk, dc = load_reference()
    import attrs

    log = []
    sk.np = _NpProxy(log)
    orig_flip, orig_erase = sk.apply_flip_augmentation_skia, sk._apply_random_erase
    cur = {}

    def flip_wrapper(image, instances, **k):
        out = orig_flip(image, instances, **k)
        cur["flip"] = out[0] is not image
        return out

    def erase_wrapper(image, *a):
        st = np.random.get_state()
        r0 = orig_erase(np.zeros_like(image), *a)
        np.random.set_state(st)
        r1 = orig_erase(np.full_like(image, 255), *a)
        np.random.set_state(st)
        out = orig_erase(image, *a)
        mask = (r0 != 0).any(-1) | (r1 != 255).any(-1)
        if mask.any():
            ys, xs = np.nonzero(mask)
            cur["erase"] = [int(ys.min()), int(xs.min()), int(ys.max() - ys.min() + 1), int(xs.max() - xs.min() + 1)]
            cur["fill"] = r0[ys[0], xs[0]].astype(np.int32).tolist()
        return out

    sk.apply_flip_augmentation_skia, sk._apply_random_erase = flip_wrapper, erase_wrapper

    z = {"intensity_defaults_json": json.dumps(attrs.asdict(dc.IntensityConfig())), "geometric_defaults_json": json.dumps(attrs.asdict(dc.GeometricConfig())),
         "configs_json": json.dumps({k: {"channels": v[0], "hw": list(v[1]), "intensity": v[2], "geometric": v[3], "symmetric": v[4]} for k, v in CONFIGS.items()}),
         "seeds": np.array(SEEDS), "samples": np.array(SAMPLES)}
    g = np.random.RandomState(1234)
    for name, (ch, (h, w), icfg, gcfg, sym) in CONFIGS.items():
        for seed in SEEDS:
            kp = (g.rand(SAMPLES, 2, 4, 2) * [w - 1, h - 1]).astype(np.float32)
            kp[:, 1, 2] = np.nan
            np.random.seed(seed)
            mats, flips, warps, erases, fills, contrast, bright, mapped = [], [], [], [], [], [], [], []
            for s in range(SAMPLES):
                img = torch.from_numpy(g.randint(0, 256, (1, ch, h, w)).astype(np.uint8))
                inst = torch.from_numpy(kp[s : s + 1].copy())
                log.clear()
                cur.clear()
                RECORD["matrix"] = None
                img, inst = sk.apply_intensity_augmentation_skia(img, inst, **icfg)
                img, inst = sk.apply_geometric_augmentation_skia(img, inst, symmetric_inds=sym, **gcfg)
                contrast.append(next((float(r) for fn, line, r in log if "contrast_min" in line), np.nan))
                bright.append(next((float(r) for fn, line, r in log if "brightness_min" in line), np.nan))
                flips.append(bool(cur.get("flip", False)))
                warps.append(RECORD["matrix"] is not None)
                mats.append(RECORD["matrix"] if RECORD["matrix"] is not None else np.array([1, 0, 0, 0, 1, 0], np.float32))
                erases.append(cur.get("erase", [-1, -1, -1, -1]))
                f = cur.get("fill", [-1] * ch)
                fills.append(f + [-1] * (3 - len(f)))
                mapped.append(inst.numpy()[0])
            key, pos = np.random.get_state()[1], np.random.get_state()[2]
            p = f"{name}/s{seed}/"
            z[p + "keypoints"] = kp
            z[p + "matrix"] = np.array(mats, np.float32)
            z[p + "warp"] = np.array(warps)
            z[p + "flip"] = np.array(flips)
            z[p + "erase"] = np.array(erases, np.int32)
            z[p + "fill"] = np.array(fills, np.int32)
            z[p + "contrast"] = np.array(contrast, np.float64)
            z[p + "brightness"] = np.array(bright, np.float64)
            z[p + "mapped"] = np.array(mapped, np.float32)
            z[p + "state_key"] = np.asarray(key, np.uint32)
            z[p + "state_pos"] = np.array(pos)
    # full intensity outputs (pure NumPy in the reference) for contrast / brightness
    for i, (ch, seed) in enumerate(((1, 3), (3, 5), (1, 11), (3, 13))):
        img = torch.from_numpy(g.randint(0, 256, (1, ch, 12, 20)).astype(np.uint8))
        img[0, 0, 0, :16] = torch.arange(0, 256, 16, dtype=torch.uint8)
        np.random.seed(seed)
        log.clear()
        out, _ = sk.apply_intensity_augmentation_skia(img, torch.zeros(1, 1, 2), contrast_min=0.3, contrast_max=2.5, contrast_p=1.0, brightness_min=0.2,
                                                      brightness_max=1.9, brightness_p=1.0 if i != 2 else 0.0)
        z[f"intensity/{i}/input"] = img.numpy()
        z[f"intensity/{i}/output"] = out.numpy()
        z[f"intensity/{i}/contrast"] = np.array(next(float(r) for fn, line, r in log if "contrast_min" in line))
        z[f"intensity/{i}/brightness"] = np.array(next((float(r) for fn, line, r in log if "brightness_min" in line), np.nan))
    np.savez_compressed(out_path, **z)
    print(out_path, os.path.getsize(out_path), "bytes")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "augment_draws.npz"))
