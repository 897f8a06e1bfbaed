"""Training augmentation on the GPU: intensity, flip, affine and erase for a whole batch in one launch.

The reference augments one sample at a time on the CPU through skia (``sleap_nn/data/skia_augmentation.py``:
``apply_intensity_augmentation_skia``, ``apply_flip_augmentation_skia``, ``apply_geometric_augmentation_skia``,
``_transform_keypoints_tensor``, ``_apply_random_erase``; called at ``data/custom_datasets.py:1101-1117`` after
pad-to-stride).  Here the per-sample scalars are drawn on the host in the reference's order and one ``ph_augment``
launch applies them to a device batch ``(B, C, H, W)``.  Contract:

* Order per sample: intensity (uniform noise, Gaussian noise, contrast, brightness), then geometric (flip, affine,
  erase).  The affine centre is ``(w/2, h/2)`` of the (padded) frame.
* Intensity in uint8 space with the reference's truncating casts (skia_augmentation.py:139-169): uniform noise is an
  integer in ``[int(min*255), int(max*255)]``; Gaussian noise ``trunc(N(mean*255, std*255))``; both added in int16 and
  clipped; contrast ``uint8(clip((v-127.5)*c + 127.5))`` then brightness ``uint8(clip(v*b))`` in float32.  float32
  frames are quantised ``(x*255).astype(uint8)`` on the way in and divided by 255 on the way out.
* Flip (skia_augmentation.py:31-95): exact mirror; keypoints ``x' = (W-1) - x``, then the symmetric pairs swap, in order.
* Affine (skia_augmentation.py:276-322): skia ``Matrix`` semantics in float32, ``M = R(angle, cx, cy) S(s, cx, cy) T(tx, ty)``
  by ``preConcat`` (independent probabilities) or ``setRotate`` / ``preScale`` / ``preTranslate`` (bundled ``affine_p``).
  Keypoints are mapped by ``M`` directly (``mapPoints`` on raw coordinates, NaN kept).  The image follows skia's
  pixel-centre convention: output pixel ``(x, y)`` is the bilinear clamp-to-edge sample at ``M^-1 (x+0.5, y+0.5) - 0.5``
  (index coordinates) times the pixel's area inside ``M [0,W]x[0,H]`` (anti-aliased ``drawImage`` over a black clear),
  rounded to nearest.  The half-pixel offset between image and keypoints is the reference's own and is kept.  A sample
  without a transform is copied, not resampled.
* Erase (skia_augmentation.py:331-335, 472-501): after the warp, ``[y, y+eh) x [x, x+ew)`` takes one fill value per channel;
  skipped when ``eh >= h`` or ``ew >= w``.
* ``mixup_*`` keys are accepted and ignored, as in the reference; only 1- or 3-channel frames; no masks.

Random draws: a ``numpy.random.RandomState`` (default: the global ``np.random``) gives the per-sample scalars in the
reference's order and with its short-circuits (a probability is drawn only when its ``p > 0``, a value only when that
draw fires; erase draws scale, ratio, ``randint`` y, ``randint`` x, ``randint(0, 256, C)`` fill).  With noise off a seeded
``Augmenter`` therefore draws what the reference's dataset draws for the same seed.  Per-pixel noise cannot follow
NumPy's stream on the device: it comes from a counter-based hash in the kernel keyed by ``(seed, sample, channel,
source y, source x)``, and the batch seed is one ``randint`` from the same RandomState after the batch's draws, taken
only when some sample's noise fired -- so the NumPy sequence diverges from the reference after the first noisy sample.
"""
from __future__ import annotations

import ctypes as C
import math
import os
import warnings
from dataclasses import dataclass, field
from typing import Any, Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from sleap_nn_amd import _lib as L

# attrs defaults of IntensityConfig / GeometricConfig (sleap_nn/config/data_config.py:195-285): what
# OmegaConf.structured fills in for keys a training config leaves out (custom_datasets.py:446-462)
INTENSITY_DEFAULTS: Dict[str, Any] = {
    "uniform_noise_min": 0.0, "uniform_noise_max": 0.04, "uniform_noise_p": 0.0,
    "gaussian_noise_mean": 0.0, "gaussian_noise_std": 0.02, "gaussian_noise_p": 0.0,
    "contrast_min": 0.9, "contrast_max": 1.1, "contrast_p": 0.0,
    "brightness_min": 0.9, "brightness_max": 1.1, "brightness_p": 0.0,
}
GEOMETRIC_DEFAULTS: Dict[str, Any] = {
    "rotation_min": -15.0, "rotation_max": 15.0, "rotation_p": 1.0,
    "scale_min": 0.9, "scale_max": 1.1, "scale_p": 1.0,
    "translate_width": 0.0, "translate_height": 0.0, "translate_p": None, "affine_p": 0.0,
    "erase_scale_min": 0.0001, "erase_scale_max": 0.01, "erase_ratio_min": 1.0, "erase_ratio_max": 1.0, "erase_p": 0.0,
    "mixup_lambda_min": 0.01, "mixup_lambda_max": 0.05, "mixup_p": 0.0, "flip_p": 0.0,
}
_F32 = np.float32


# ---------------------------------------------------------------------------------------------------------------------
# skia Matrix arithmetic (affine part), float32 like SkScalar: [sx, kx, tx, ky, sy, ty]
# ---------------------------------------------------------------------------------------------------------------------
def _identity() -> np.ndarray:
    return np.array([1, 0, 0, 0, 1, 0], dtype=_F32)


def _snap(v: np.float32) -> np.float32:
    return _F32(0.0) if abs(float(v)) <= 1.0 / 4096 else v  # SkScalarSinSnapToZero / CosSnapToZero


def _rotate(degrees: float, px: float, py: float) -> np.ndarray:
    """SkMatrix::setRotate(degrees, px, py)."""
    rad = _F32(degrees) * _F32(math.pi / 180.0)
    s, c = _snap(np.sin(rad, dtype=_F32)), _snap(np.cos(rad, dtype=_F32))
    px, py = _F32(px), _F32(py)
    one_c = _F32(1) - c
    return np.array([c, -s, s * py + one_c * px, s, c, -s * px + one_c * py], dtype=_F32)


def _scale(sx: float, sy: float, px: float, py: float) -> np.ndarray:
    """SkMatrix::setScale(sx, sy, px, py)."""
    sx, sy, px, py = _F32(sx), _F32(sy), _F32(px), _F32(py)
    if sx == 1 and sy == 1:
        return _identity()
    return np.array([sx, 0, px - sx * px, 0, sy, py - sy * py], dtype=_F32)


def _translate(dx: float, dy: float) -> np.ndarray:
    return np.array([1, 0, _F32(dx), 0, 1, _F32(dy)], dtype=_F32)


def _concat(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """SkMatrix::setConcat(a, b) for affine matrices (muladdmul in double, rounded to float)."""
    def mam(p, q, r, s):
        return _F32(float(p) * float(q) + float(r) * float(s))

    return np.array([mam(a[0], b[0], a[1], b[3]), mam(a[0], b[1], a[1], b[4]), mam(a[0], b[2], a[1], b[5]) + a[2],
                     mam(a[3], b[0], a[4], b[3]), mam(a[3], b[1], a[4], b[4]), mam(a[3], b[2], a[4], b[5]) + a[5]], dtype=_F32)


def _pre_translate(m: np.ndarray, dx: float, dy: float) -> np.ndarray:
    """SkMatrix::preTranslate(dx, dy)."""
    dx, dy = _F32(dx), _F32(dy)
    out = m.copy()
    if m[0] == 1 and m[1] == 0 and m[3] == 0 and m[4] == 1:
        out[2] = m[2] + dx
        out[5] = m[5] + dy
    else:
        out[2] = m[2] + (m[0] * dx + m[1] * dy)
        out[5] = m[5] + (m[3] * dx + m[4] * dy)
    return out


def map_points(m: np.ndarray, pts: np.ndarray) -> np.ndarray:
    """SkMatrix::mapPoints on (..., 2) float32 points (x sx + y kx) + tx; NaN rows stay NaN."""
    p = np.asarray(pts, dtype=_F32)
    x, y = p[..., 0], p[..., 1]
    out = np.empty_like(p)
    out[..., 0] = (x * m[0] + y * m[1]) + m[2]
    out[..., 1] = (x * m[3] + y * m[4]) + m[5]
    return out


# ---------------------------------------------------------------------------------------------------------------------
# host draws
# ---------------------------------------------------------------------------------------------------------------------
@dataclass
class SampleDraw:
    """What the reference would have drawn for one sample (plus what the kernel needs)."""

    uniform: bool = False
    gaussian: bool = False
    contrast: Optional[float] = None
    brightness: Optional[float] = None
    flip: bool = False
    warp: bool = False
    matrix: np.ndarray = field(default_factory=_identity)  # skia matrix [sx, kx, tx, ky, sy, ty], float32
    erase: Optional[Tuple[int, int, int, int]] = None  # (y, x, eh, ew)
    fill: Optional[np.ndarray] = None  # uint8 (C,)


def _merged(defaults: Dict[str, Any], cfg: Optional[Dict[str, Any]], what: str) -> Dict[str, Any]:
    cfg = dict(cfg or {})
    unknown = set(cfg) - set(defaults)
    if unknown:
        raise ValueError(f"unknown {what} augmentation keys: {sorted(unknown)}")
    return {**defaults, **cfg}


def _draw_intensity(rng, cfg: Dict[str, Any], d: SampleDraw) -> None:
    """skia_augmentation.py:139-169, without the per-pixel noise arrays."""
    if cfg["uniform_noise_p"] > 0 and rng.random() < cfg["uniform_noise_p"]:
        d.uniform = True
    if cfg["gaussian_noise_p"] > 0 and rng.random() < cfg["gaussian_noise_p"]:
        d.gaussian = True
    if cfg["contrast_p"] > 0 and rng.random() < cfg["contrast_p"]:
        d.contrast = float(rng.uniform(cfg["contrast_min"], cfg["contrast_max"]))
    if cfg["brightness_p"] > 0 and rng.random() < cfg["brightness_p"]:
        d.brightness = float(rng.uniform(cfg["brightness_min"], cfg["brightness_max"]))


def _draw_geometric(rng, cfg: Dict[str, Any], h: int, w: int, channels: int, d: SampleDraw) -> None:
    """skia_augmentation.py:247-335 (with the flip of :30-95 and the erase of :472-501)."""
    if cfg["flip_p"] > 0 and not rng.random() >= cfg["flip_p"]:
        d.flip = True
    cx, cy = w / 2, h / 2
    m = _identity()
    rp, sp, tp = cfg["rotation_p"], cfg["scale_p"], cfg["translate_p"]
    if rp is not None or sp is not None or tp is not None:
        if rp is not None and rp > 0 and rng.random() < rp:
            m = _concat(m, _rotate(rng.uniform(cfg["rotation_min"], cfg["rotation_max"]), cx, cy))
            d.warp = True
        if sp is not None and sp > 0 and rng.random() < sp:
            s = rng.uniform(cfg["scale_min"], cfg["scale_max"])
            m = _concat(m, _scale(s, s, cx, cy))
            d.warp = True
        if tp is not None and tp > 0 and rng.random() < tp:
            tx = rng.uniform(-cfg["translate_width"], cfg["translate_width"]) * w
            ty = rng.uniform(-cfg["translate_height"], cfg["translate_height"]) * h
            m = _concat(m, _translate(tx, ty))
            d.warp = True
    elif cfg["affine_p"] > 0 and rng.random() < cfg["affine_p"]:
        angle = rng.uniform(cfg["rotation_min"], cfg["rotation_max"])
        s = rng.uniform(cfg["scale_min"], cfg["scale_max"])
        tx = rng.uniform(-cfg["translate_width"], cfg["translate_width"]) * w
        ty = rng.uniform(-cfg["translate_height"], cfg["translate_height"]) * h
        m = _rotate(angle, cx, cy)
        if not (_F32(s) == 1):
            m = _concat(m, _scale(s, s, cx, cy))
        m = _pre_translate(m, tx, ty)
        d.warp = True
    d.matrix = m
    if cfg["erase_p"] > 0 and rng.random() < cfg["erase_p"]:
        area = h * w
        erase_area = rng.uniform(cfg["erase_scale_min"], cfg["erase_scale_max"]) * area
        ratio = rng.uniform(cfg["erase_ratio_min"], cfg["erase_ratio_max"])
        eh, ew = int(np.sqrt(erase_area * ratio)), int(np.sqrt(erase_area / ratio))
        if eh < h and ew < w:
            y = int(rng.randint(0, h - eh))
            x = int(rng.randint(0, w - ew))
            d.fill = rng.randint(0, 256, size=(channels,), dtype=np.uint8)
            d.erase = (y, x, eh, ew)


def _pack(draws: Sequence[SampleDraw], h: int, w: int, intensity: Optional[Dict[str, Any]], seed: int):
    arr = (L.AugSample * len(draws))()
    for a, d in zip(arr, draws):
        flags = 0
        if intensity is not None:
            if d.uniform:
                flags |= L.AUG_UNIFORM
                a.uni_lo, a.uni_hi = int(intensity["uniform_noise_min"] * 255), int(intensity["uniform_noise_max"] * 255)
                if a.uni_hi < a.uni_lo:
                    raise ValueError("uniform_noise_max < uniform_noise_min")
            if d.gaussian:
                flags |= L.AUG_GAUSS
                a.gauss_mean, a.gauss_std = intensity["gaussian_noise_mean"] * 255, intensity["gaussian_noise_std"] * 255
        if d.contrast is not None:
            flags |= L.AUG_CONTRAST
            a.contrast = d.contrast
        if d.brightness is not None:
            flags |= L.AUG_BRIGHTNESS
            a.brightness = d.brightness
        if d.flip:
            flags |= L.AUG_FLIP
        m = d.matrix.astype(np.float64)
        a.m[:] = [float(v) for v in d.matrix]
        if d.warp:
            flags |= L.AUG_WARP
            A = np.array([[m[0], m[1]], [m[3], m[4]]])
            det = float(np.linalg.det(A))
            if abs(det) < 1e-12:  # degenerate map: nothing of the frame is drawn
                a.edge[:] = [0.0, 0.0, -1.0] * 4
            else:
                Ai = np.linalg.inv(A)
                t = -Ai @ np.array([m[2], m[5]])
                inv = np.array([Ai[0, 0], Ai[0, 1], t[0], Ai[1, 0], Ai[1, 1], t[1]])
                if d.flip:  # mirror of the source about its centre: x -> W - x (pixel coordinates)
                    inv[0:3] = [-inv[0], -inv[1], w - inv[2]]
                a.minv[:] = [float(v) for v in inv]
                corners = [(m[0] * x + m[1] * y + m[2], m[3] * x + m[4] * y + m[5]) for x, y in ((0, 0), (w, 0), (w, h), (0, h))]
                ctr = np.mean(corners, axis=0)
                e = []
                for k in range(4):
                    (x0, y0), (x1, y1) = corners[k], corners[(k + 1) % 4]
                    nx, ny = -(y1 - y0), x1 - x0
                    nn = math.hypot(nx, ny)
                    nx, ny = nx / nn, ny / nn
                    dd = -(nx * x0 + ny * y0)
                    if nx * ctr[0] + ny * ctr[1] + dd < 0:
                        nx, ny, dd = -nx, -ny, -dd
                    e += [nx, ny, dd]
                a.edge[:] = e
        if d.erase is not None:
            flags |= L.AUG_ERASE
            a.erase_y, a.erase_x, a.erase_h, a.erase_w = d.erase
            f = [int(v) for v in d.fill] + [0] * (3 - len(d.fill))
            a.fill[:] = f[:3]
        a.flags = flags
        a.seed = seed & 0xFFFFFFFF
    return arr


def _check_image(image: torch.Tensor) -> Tuple[int, int, int, int]:
    L.require_cuda(image, "image")
    if image.dim() != 4:
        raise ValueError(f"image must be (B, C, H, W), got {tuple(image.shape)}")
    if image.dtype not in (torch.uint8, torch.float32):
        raise ValueError(f"image must be uint8 or float32, got {image.dtype}")
    B, Cc, H, W = image.shape
    if Cc not in (1, 3):
        raise ValueError(f"Unsupported channels: {Cc} (the reference's skia path takes 1 or 3)")
    return B, Cc, H, W


def _launch(image: torch.Tensor, instances: Optional[torch.Tensor], params, symmetric_inds=(), counters: Optional[torch.Tensor] = None):
    """One ph_augment call with explicit per-sample parameters (an ``AugSample`` array of length B)."""
    B, Cc, H, W = _check_image(image)
    dev = image.device
    src = image.contiguous()
    out = torch.empty_like(src)
    raw = np.frombuffer(bytes(params), dtype=np.uint8)
    if raw.size != B * C.sizeof(L.AugSample):
        raise ValueError(f"{raw.size // C.sizeof(L.AugSample)} parameter records for a batch of {B}")
    # one H2D per batch from pinned staging (torch's host allocator keeps the block until the copy has completed)
    p_dev = torch.from_numpy(raw.copy()).pin_memory().to(dev, non_blocking=True)
    kin = kout = None
    I = N = 0
    if instances is not None:
        L.require_cuda(instances, "instances")
        if instances.shape[0] != B or instances.shape[-1] != 2 or instances.dim() not in (3, 4):
            raise ValueError(f"instances must be (B, I, N, 2) or (B, N, 2), got {tuple(instances.shape)}")
        kin = instances.to(torch.float32).contiguous()
        kout = torch.empty_like(kin)
        N = int(kin.shape[-2])
        I = int(kin.shape[1]) if kin.dim() == 4 else 1
    pairs = torch.tensor([list(p) for p in symmetric_inds], dtype=torch.int32).reshape(-1, 2)
    if pairs.numel() and (int(pairs.min()) < 0 or int(pairs.max()) >= max(N, 1)):
        raise ValueError(f"symmetric pair index out of range for {N} nodes")
    pairs = pairs.to(dev).contiguous()
    with torch.cuda.device(dev):
        L.check(L.lib().ph_augment(C.c_void_p(src.data_ptr()), C.c_void_p(out.data_ptr()), 0 if src.dtype == torch.uint8 else 1, B, Cc, H, W,
                                   C.c_void_p(kin.data_ptr()) if kin is not None else None, C.c_void_p(kout.data_ptr()) if kout is not None else None,
                                   I, N, C.c_void_p(p_dev.data_ptr()), C.c_void_p(pairs.data_ptr()) if pairs.numel() else None, int(pairs.shape[0]),
                                   C.c_void_p(counters.data_ptr()) if counters is not None else None, L.current_stream_ptr()))
    return out, (kout.to(instances.dtype) if kout is not None else None)


def _rng(rng):
    return np.random if rng is None else rng


def _draw_batch(rng, B: int, h: int, w: int, channels: int, intensity: Optional[Dict[str, Any]], geometric: Optional[Dict[str, Any]]):
    draws = []
    for _ in range(B):
        d = SampleDraw()
        if intensity is not None:
            _draw_intensity(rng, intensity, d)
        if geometric is not None:
            _draw_geometric(rng, geometric, h, w, channels, d)
        draws.append(d)
    seed = int(rng.randint(0, 2**31 - 1)) if any(d.uniform or d.gaussian for d in draws) else 0
    return draws, seed


# ---------------------------------------------------------------------------------------------------------------------
# public functions (the reference's keyword names and defaults, batched)
# ---------------------------------------------------------------------------------------------------------------------
def apply_intensity_augmentation(image: torch.Tensor, instances: torch.Tensor, uniform_noise_min: float = 0.0, uniform_noise_max: float = 0.04,
                                 uniform_noise_p: float = 0.0, gaussian_noise_mean: float = 0.0, gaussian_noise_std: float = 0.02,
                                 gaussian_noise_p: float = 0.0, contrast_min: float = 0.9, contrast_max: float = 1.1, contrast_p: float = 0.0,
                                 brightness_min: float = 0.9, brightness_max: float = 1.1, brightness_p: float = 0.0, rng=None):
    """Intensity augmentation of a device batch ``(B, C, H, W)``; instances pass through (copied)."""
    cfg = dict(uniform_noise_min=uniform_noise_min, uniform_noise_max=uniform_noise_max, uniform_noise_p=uniform_noise_p, gaussian_noise_mean=gaussian_noise_mean,
               gaussian_noise_std=gaussian_noise_std, gaussian_noise_p=gaussian_noise_p, contrast_min=contrast_min, contrast_max=contrast_max, contrast_p=contrast_p,
               brightness_min=brightness_min, brightness_max=brightness_max, brightness_p=brightness_p)
    B, Cc, H, W = _check_image(image)
    draws, seed = _draw_batch(_rng(rng), B, H, W, Cc, cfg, None)
    out, _ = _launch(image, None, _pack(draws, H, W, cfg, seed))
    return out, (instances.clone() if instances is not None else None)


def apply_geometric_augmentation(image: torch.Tensor, instances: torch.Tensor, rotation_min: float = -15.0, rotation_max: float = 15.0,
                                 rotation_p: Optional[float] = None, scale_min: float = 0.9, scale_max: float = 1.1, scale_p: Optional[float] = None,
                                 translate_width: float = 0.02, translate_height: float = 0.02, translate_p: Optional[float] = None, affine_p: float = 0.0,
                                 erase_scale_min: float = 0.0001, erase_scale_max: float = 0.01, erase_ratio_min: float = 1.0, erase_ratio_max: float = 1.0,
                                 erase_p: float = 0.0, mixup_lambda_min: float = 0.01, mixup_lambda_max: float = 0.05, mixup_p: float = 0.0, flip_p: float = 0.0,
                                 symmetric_inds: Optional[Sequence[Tuple[int, int]]] = None, rng=None):
    """Flip, affine and erase of a device batch ``(B, C, H, W)`` and its keypoints ``(B, I, N, 2)`` / ``(B, N, 2)``.
    ``mixup_*`` is accepted and ignored, as in the reference."""
    cfg = dict(rotation_min=rotation_min, rotation_max=rotation_max, rotation_p=rotation_p, scale_min=scale_min, scale_max=scale_max, scale_p=scale_p,
               translate_width=translate_width, translate_height=translate_height, translate_p=translate_p, affine_p=affine_p, erase_scale_min=erase_scale_min,
               erase_scale_max=erase_scale_max, erase_ratio_min=erase_ratio_min, erase_ratio_max=erase_ratio_max, erase_p=erase_p, mixup_lambda_min=mixup_lambda_min,
               mixup_lambda_max=mixup_lambda_max, mixup_p=mixup_p, flip_p=flip_p)
    B, Cc, H, W = _check_image(image)
    draws, seed = _draw_batch(_rng(rng), B, H, W, Cc, None, cfg)
    return _launch(image, instances, _pack(draws, H, W, None, seed), symmetric_inds or ())


def apply_flip_augmentation(image: torch.Tensor, instances: torch.Tensor, symmetric_inds: Optional[Sequence[Tuple[int, int]]] = None, flip_p: float = 0.0, rng=None):
    """Left/right mirror of each sample with probability ``flip_p`` (one draw per sample), symmetric pairs swapped."""
    B, Cc, H, W = _check_image(image)
    r = _rng(rng)
    draws = [SampleDraw(flip=bool(flip_p > 0 and not r.random() >= flip_p)) for _ in range(B)]
    return _launch(image, instances, _pack(draws, H, W, None, 0), symmetric_inds or ())


class Augmenter:
    """The reference's training augmentation for whole device batches.

    ``intensity`` / ``geometric``: ``IntensityConfig`` / ``GeometricConfig`` fields (missing keys take their attrs defaults,
    ``None`` disables the stage); ``symmetric_inds``: node pairs swapped after a flip; ``rng``: a
    ``numpy.random.RandomState`` (default: the global ``np.random``).  ``augmenter(image, instances)`` draws the B samples'
    parameters in the reference's order and runs one ``ph_augment`` launch."""

    def __init__(self, intensity: Optional[Dict[str, Any]] = None, geometric: Optional[Dict[str, Any]] = None, symmetric_inds: Sequence[Tuple[int, int]] = (),
                 rng=None) -> None:
        self.intensity = _merged(INTENSITY_DEFAULTS, intensity, "intensity") if intensity is not None else None
        self.geometric = _merged(GEOMETRIC_DEFAULTS, geometric, "geometric") if geometric is not None else None
        self.symmetric_inds = [tuple(int(i) for i in p) for p in symmetric_inds]
        self.rng = rng

    def draw(self, n: int, hw: Tuple[int, int], channels: int = 1) -> Tuple[List[SampleDraw], int]:
        """The parameters of n samples of an ``hw`` frame (what ``__call__`` uses), and the noise seed (0 without noise)."""
        if channels not in (1, 3):
            raise ValueError(f"Unsupported channels: {channels} (the reference's skia path takes 1 or 3)")
        return _draw_batch(_rng(self.rng), n, int(hw[0]), int(hw[1]), channels, self.intensity, self.geometric)

    def __call__(self, image: torch.Tensor, instances: Optional[torch.Tensor] = None, counters: Optional[torch.Tensor] = None):
        B, Cc, H, W = _check_image(image)
        draws, seed = self.draw(B, (H, W), Cc)
        return _launch(image, instances, _pack(draws, H, W, self.intensity, seed), self.symmetric_inds, counters)

    @classmethod
    def from_training_config(cls, cfg_or_path, rng=None) -> "Augmenter":
        """From a sleap-nn training config (dict or YAML path): ``data_config.use_augmentations_train`` and
        ``data_config.augmentation_config``; symmetric pairs from the first skeleton's ``symmetries``."""
        cfg = cfg_or_path
        if isinstance(cfg, (str, os.PathLike)):
            import yaml

            with open(cfg) as f:
                cfg = yaml.safe_load(f)
        data = cfg.get("data_config", cfg) or {}
        sym = _symmetric_inds((data.get("skeletons") or [None])[0])
        if not data.get("use_augmentations_train", False):
            return cls(None, None, sym, rng)
        aug = data.get("augmentation_config") or {}
        aug_obj = cls(aug.get("intensity"), aug.get("geometric"), sym, rng)
        if aug_obj.geometric is not None and aug_obj.geometric["flip_p"] and aug_obj.geometric["flip_p"] > 0 and not sym:
            warnings.warn("Flip augmentation is enabled (flip_p > 0) but the skeleton has no symmetries. Flipping will not swap any nodes, which is only "
                          "correct if the labeled animal is truly left/right symmetric. Add symmetry pairs to the skeleton to fix this.", stacklevel=2)
        return aug_obj

    @classmethod
    def from_run_dir(cls, run_dir: str, rng=None) -> "Augmenter":
        return cls.from_training_config(os.path.join(run_dir, "training_config.yaml"), rng)


def _symmetric_inds(skeleton: Optional[Dict[str, Any]]) -> List[Tuple[int, int]]:
    """data/utils.py:22-52: node-index pairs of the skeleton's symmetries (empty when there are none)."""
    if not skeleton:
        return []
    names = [n["name"] if isinstance(n, dict) else str(n) for n in skeleton.get("nodes") or []]

    def name(v):
        return v["name"] if isinstance(v, dict) else str(v)

    pairs = []
    for s in skeleton.get("symmetries") or []:
        a, b = list(s)
        pairs.append((names.index(name(a)), names.index(name(b))))
    return pairs
