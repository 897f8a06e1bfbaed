"""Seeded frames for the optical-flow tests and ``tools/gen_tracking_flow_golden.py``: the golden holds results and parameters only, the frames come from here.

``texture(seed, h, w, shift)``: a band-limited texture of 40 random sinusoids with wavelengths 6 to 48 px, evaluated at ``(x - dx, y - dy)`` -- the scene moved
by ``shift = (dx, dy)`` pixels, exactly, at any sub-pixel amount -- and quantised to uint8.  ``scene_frames`` moves one texture along a list of shifts.
"""
from __future__ import annotations

import numpy as np

N_WAVES = 40


def texture(seed: int, h: int, w: int, shift=(0.0, 0.0), flat=None) -> np.ndarray:
    """uint8 (h, w).  ``flat = (y0, y1, x0, x1)``: that rectangle is set to the constant 128 (a region without gradient)."""
    g = np.random.default_rng(seed)
    lam = g.uniform(6.0, 48.0, N_WAVES)
    ang = g.uniform(0.0, 2 * np.pi, N_WAVES)
    phase = g.uniform(0.0, 2 * np.pi, N_WAVES)
    amp = g.uniform(0.5, 1.0, N_WAVES)
    kx, ky = 2 * np.pi / lam * np.cos(ang), 2 * np.pi / lam * np.sin(ang)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    xx, yy = xx - float(shift[0]), yy - float(shift[1])
    v = np.zeros((h, w))
    for i in range(N_WAVES):
        v += amp[i] * np.sin(kx[i] * xx + ky[i] * yy + phase[i])
    v = v / (np.sqrt(N_WAVES / 2.0) * 0.75 * 3.0)  # about +- 3 sigma into +- 1
    img = np.clip(np.rint(128.0 + 110.0 * v), 0, 255).astype(np.uint8)
    if flat is not None:
        y0, y1, x0, x1 = flat
        img[y0:y1, x0:x1] = 128
    return img


def scene_frames(seed: int, h: int, w: int, shifts) -> np.ndarray:
    """uint8 (T, h, w): the texture of ``seed`` moved by each of ``shifts`` (T, 2)."""
    return np.stack([texture(seed, h, w, s) for s in shifts])


SEQ_HW = (96, 160)


def flow_sequence(seed: int, kind: str = "plain", n_frames: int = 10, n_nodes: int = 4):
    """A tracking sequence on a moving scene: ``(frames uint8 (T, H, W), [(points (I, N, 2) float64 with NaN, detection scores (I,)) per frame])``.  The scene
    (a texture) moves by a new shift every frame, the animals ride on it with a little motion of their own, the instance order is shuffled per frame.

    ``plain``: three animals, jittery scene shifts of up to (7, 4) px per frame, some dropouts and missing nodes.
    ``sparse``: as plain with 40 % missing nodes (instances at and below a ``min_match_points`` floor occur).
    ``lost``: the scene drifts steadily, animals near the border leave the frame: their flow is lost (NaN).
    ``surplus``: as plain without dropouts, and in most frames near-copies of an animal are added (the pre-cull's input).
    ``close``: two animals 6 px apart along x while the scene moves 6 px along x per frame -- each lands where the other was."""
    g = np.random.default_rng(seed)
    h, w = SEQ_HW
    n_animals = 2 if kind == "close" else 3
    if kind == "close":
        steps = np.tile([[6.0, 0.5]], (n_frames, 1))
    elif kind == "lost":
        steps = np.tile([[7.0, 2.0]], (n_frames, 1)) + g.uniform(-1, 1, (n_frames, 2))
    else:
        steps = g.uniform(-1, 1, (n_frames, 2)) * np.array([7.0, 4.0])
    steps[0] = 0
    shifts = np.cumsum(steps, axis=0)
    if kind not in ("close", "lost"):
        shifts = shifts - shifts.mean(axis=0)
    frames = scene_frames(seed, h, w, shifts)
    if kind == "close":
        pos = np.array([[40.0, 45.0], [46.0, 45.0]])
        shape = np.tile(g.normal(0, 1.5, (1, n_nodes, 2)), (2, 1, 1))
    elif kind == "lost":
        pos = np.stack([g.uniform(90, 130, n_animals), g.uniform(50, 80, n_animals)], axis=1)
        shape = g.normal(0, 7, (n_animals, n_nodes, 2))
    else:
        pos = np.stack([g.uniform(45, 115, n_animals), g.uniform(35, 60, n_animals)], axis=1)
        shape = g.normal(0, 7, (n_animals, n_nodes, 2))
    vel = np.zeros((n_animals, 2))
    out = []
    for t in range(n_frames):
        if kind != "close":
            vel = 0.8 * vel + g.normal(0, 0.4, vel.shape)
            pos = pos + vel
        insts = []
        for a in range(n_animals):
            if kind in ("plain", "sparse") and t > 0 and g.uniform() < 0.1:
                continue
            pts = pos[a] + shape[a] + shifts[t] + (0 if kind == "close" else g.normal(0, 0.3, (n_nodes, 2)))
            if kind != "close":
                pts[g.uniform(size=n_nodes) < (0.4 if kind == "sparse" else 0.1)] = np.nan
            insts.append((pts, g.uniform(0.3, 1.0)))
        if kind == "surplus":
            for _ in range(int(g.integers(0, 3))):
                src = insts[int(g.integers(0, n_animals))]
                insts.append((src[0] + g.normal(0, 0.8, (n_nodes, 2)), g.uniform(0.3, 1.0)))
        order = g.permutation(len(insts)) if kind != "close" else (np.arange(2) if t % 2 == 0 else np.arange(2)[::-1])
        pts = np.stack([insts[i][0] for i in order]) if len(insts) else np.zeros((0, n_nodes, 2))
        out.append((pts, np.array([insts[i][1] for i in order], dtype=np.float64)))
    return frames, out


def interior_points(seed: int, n: int, h: int, w: int, margin: float) -> np.ndarray:
    g = np.random.default_rng(seed)
    return np.stack([g.uniform(margin, w - 1 - margin, n), g.uniform(margin, h - 1 - margin, n)], axis=1).astype(np.float32)
