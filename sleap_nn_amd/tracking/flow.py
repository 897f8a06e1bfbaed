"""Pyramidal Lucas-Kanade optical flow for the flow-shift tracker (sleap_nn/tracking/tracker.py:631-841 calls ``cv2.calcOpticalFlowPyrLK``).

``pyr_lk`` is (a) the CPU path of the tracker's ``use_flow``, (b) the STAND-IN that ``tools/gen_tracking_flow_golden.py`` hands to the reference's
``FlowShiftTracker`` as ``cv2.calcOpticalFlowPyrLK`` -- OpenCV is not a dependency of this project, and the goldens made with this function pin the tracker's
LOGIC, not OpenCV's numbers -- and (c) the specification ``ph_flow_pyramid`` / ``ph_flow_track`` (csrc/flow_kernels.hip) are tested against; ``pyramid_device``
and ``track_device`` below bind them.
"""
from __future__ import annotations

import ctypes as C
from typing import List, Sequence, Tuple

import numpy as np

MIN_WIN, MAX_WIN, MAX_LEVELS = 3, 41, 8  # ph_flow_track: win 3..41, max_level 0..7
_W_BITS = 14
_FLT_SCALE = np.float32(1.0 / (1 << 20))
_FLT_EPSILON = np.float32(1.1920928955078125e-7)
_MIN_EIG = 1e-4
_KERNEL = (1, 4, 6, 4, 1)
_LIMIT = 1.0e9  # a coordinate beyond it is outside every frame; keeps float -> int defined


def reflect101(i, n: int):
    """Index ``i`` into an axis of length ``n`` continued ``... 2 1 | 0 1 2 ... n-1 | n-2 n-3 ...`` (OpenCV's ``BORDER_REFLECT_101``), any distance."""
    i = np.asarray(i, dtype=np.int64)
    if n == 1:
        return np.zeros_like(i)
    m = 2 * (n - 1)
    i = np.mod(i, m)
    return np.where(i >= n, m - i, i)


def pyramid_shapes(h: int, w: int, win: int, max_level: int) -> List[Tuple[int, int]]:
    """``(height, width)`` of every level: level l + 1 is ``((h + 1) // 2, (w + 1) // 2)`` and exists only while both sides exceed ``win``, up to ``max_level``."""
    shapes = [(int(h), int(w))]
    while len(shapes) - 1 < max_level:
        h2, w2 = (shapes[-1][0] + 1) // 2, (shapes[-1][1] + 1) // 2
        if w2 <= win or h2 <= win:
            break
        shapes.append((h2, w2))
    return shapes


def pyr_down(img: np.ndarray) -> np.ndarray:
    """One level up: separable ``[1 4 6 4 1]`` sampled at ``(2x, 2y)``, reflect-101 borders, ``(sum + 128) >> 8`` as uint8."""
    h, w = img.shape
    h2, w2 = (h + 1) // 2, (w + 1) // 2
    src = img.astype(np.int32)
    rows = np.zeros((h, w2), dtype=np.int32)
    for d, k in enumerate(_KERNEL):
        rows += k * src[:, reflect101(2 * np.arange(w2) + d - 2, w)]
    out = np.zeros((h2, w2), dtype=np.int32)
    for d, k in enumerate(_KERNEL):
        out += k * rows[reflect101(2 * np.arange(h2) + d - 2, h), :]
    return ((out + 128) >> 8).astype(np.uint8)


def build_pyramid(img: np.ndarray, win: int = 21, max_level: int = 3) -> List[np.ndarray]:
    img = np.ascontiguousarray(img)
    if img.dtype != np.uint8 or img.ndim != 2:
        raise ValueError(f"build_pyramid: a uint8 (H, W) image is needed, got {img.dtype} {img.shape}")
    levels = [img]
    for _ in pyramid_shapes(img.shape[0], img.shape[1], win, max_level)[1:]:
        levels.append(pyr_down(levels[-1]))
    return levels


def scharr(img: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """``(Ix, Iy)`` int16 of a uint8 image, the image taken reflect-101 at its edges: ``Ix = (3 I(x+1,y-1) + 10 I(x+1,y) + 3 I(x+1,y+1)) - (same at x-1)``."""
    h, w = img.shape
    p = img.astype(np.int32)[reflect101(np.arange(-1, h + 1), h)][:, reflect101(np.arange(-1, w + 1), w)]
    smooth_y = 3 * (p[:-2] + p[2:]) + 10 * p[1:-1]  # (h, w + 2)
    smooth_x = 3 * (p[:, :-2] + p[:, 2:]) + 10 * p[:, 1:-1]  # (h + 2, w)
    return (smooth_y[:, 2:] - smooth_y[:, :-2]).astype(np.int16), (smooth_x[2:] - smooth_x[:-2]).astype(np.int16)


def _to_int(v: np.ndarray) -> np.ndarray:
    return np.clip(v, -_LIMIT, _LIMIT).astype(np.int64)


def _outside(ix, iy, w: int, h: int, win: int):
    return (ix < -win) | (ix >= w) | (iy < -win) | (iy >= h)


def _margin(v: np.ndarray, w: int, h: int, win: int, rounded: bool = False) -> np.ndarray:
    """How far (px) the tested coordinates ``v`` (n, 2) are from flipping the bounds test, floor'ed or rounded."""
    lo = -win - (0.5 if rounded else 0.0)
    hi = np.array([w, h], dtype=np.float64) - (0.5 if rounded else 0.0)
    v = v.astype(np.float64)
    return np.minimum(np.abs(v - lo), np.abs(v - hi)).min(axis=1)


def _weights(a: np.ndarray, b: np.ndarray):
    """Bilinear weights ``round(w * 2^14)`` (half to even, float32 products); the fourth is ``2^14`` minus the other three.  Shaped (P, 1, 1)."""
    one, s = np.float32(1.0), np.float32(1 << _W_BITS)
    w00 = np.rint((one - a) * (one - b) * s).astype(np.int64)
    w01 = np.rint(a * (one - b) * s).astype(np.int64)
    w10 = np.rint((one - a) * b * s).astype(np.int64)
    w11 = (1 << _W_BITS) - w00 - w01 - w10
    return tuple(v[:, None, None] for v in (w00, w01, w10, w11))


def _blend(patch: np.ndarray, wts, shift: int) -> np.ndarray:
    """(P, win + 1, win + 1) integers -> (P, win, win): ``(sum of the four corners times their weights + 2^(shift - 1)) >> shift``."""
    w00, w01, w10, w11 = wts
    return (patch[:, :-1, :-1] * w00 + patch[:, :-1, 1:] * w01 + patch[:, 1:, :-1] * w10 + patch[:, 1:, 1:] * w11 + (1 << (shift - 1))) >> shift


def _patch(img: np.ndarray, ix: np.ndarray, iy: np.ndarray, win: int, zero_outside: bool) -> np.ndarray:
    """(P, win + 1, win + 1) int64 samples with top-left ``(ix, iy)``; outside the image: reflect-101 (the image) or 0 (a derivative)."""
    h, w = img.shape
    ys = iy[:, None] + np.arange(win + 1)[None, :]
    xs = ix[:, None] + np.arange(win + 1)[None, :]
    if zero_outside:
        inside = ((ys >= 0) & (ys < h))[:, :, None] & ((xs >= 0) & (xs < w))[:, None, :]
        return img[np.clip(ys, 0, h - 1)[:, :, None], np.clip(xs, 0, w - 1)[:, None, :]].astype(np.int64) * inside
    return img[reflect101(ys, h)[:, :, None], reflect101(xs, w)[:, None, :]].astype(np.int64)


def pyr_lk(ref_img: np.ndarray, new_img: np.ndarray, pts: np.ndarray, win: int = 21, max_level: int = 3, max_iter: int = 30, eps: float = 0.01,
           ref_pyramid: Sequence[np.ndarray] = None, new_pyramid: Sequence[np.ndarray] = None, info: dict = None) -> Tuple[np.ndarray, np.ndarray]:
    """Where the points ``pts`` (P, 2) (x, y) of ``ref_img`` lie on ``new_img``: ``(shifted (P, 2) float32, status (P,) uint8)``.  uint8 grayscale ``(H, W)``
    images; every point is worked at once (NumPy over the points), each by the recurrence below.  A STAND-IN for ``cv2.calcOpticalFlowPyrLK(ref, new, pts, None,
    winSize=(win, win), maxLevel=max_level, criteria=(EPS | COUNT, max_iter, eps))`` in OpenCV's integer arithmetic as far as it is stated here, NOT a pin of
    OpenCV's output: this docstring is the contract, and the kernels are bound to it by the tests.  (``ref_pyramid`` / ``new_pyramid``: levels built before;
    ``info``: a dict that receives ``min_eig`` (P, levels), NaN where none was computed, and ``margin`` (P,), the least distance in px of any bounds test of the
    point from flipping -- what a test needs to pick points whose status does not hang on the last bit.)

    Pyramid.  Level 0 is the image; level l + 1 has size ``((w + 1) // 2, (h + 1) // 2)`` and is added only while both of its sides exceed ``win``, and only up
    to ``max_level``.  Downsampling is separable ``[1 4 6 4 1]`` sampled at ``(2x, 2y)`` with reflect-101 borders; the result is ``(sum + 128) >> 8`` as uint8.

    Derivatives.  Scharr, int16: ``Ix = (3 I(x+1,y-1) + 10 I(x+1,y) + 3 I(x+1,y+1)) - (the same at x-1)``, ``Iy`` its transpose; at image edges the image is taken
    reflect-101.  Outside the image the derivatives are 0, while the image itself continues reflect-101.

    Per point, from the coarsest level down.  ``prev = pt / 2^l``; the guess ``next`` is ``prev`` at the top level and twice the level above's result otherwise
    (a level that is skipped hands its guess on).  ``half = (win - 1) / 2``; the window's top-left is ``prev - half``.  If ``floor(prev - half)`` is ``< -win`` or
    ``>=`` the level's width or height the point is skipped at this level; at level 0 that sets ``status = 0``.

    Patch sampling, fixed point.  Bilinear weights are ``round(w * 2^14)`` (half to even; products in float32), the fourth ``2^14`` minus the other three.  Image
    patches are ``(sum + 2^8) >> 9`` (32 x the pixel value), derivative patches ``(sum + 2^13) >> 14``.

    Normal matrix and status.  ``A11, A12, A22`` are the sums over the window of the integer products (exact integer sums, then float32) times ``2^-20``;
    ``D = A11 A22 - A12^2``; ``minEig = (A22 + A11 - sqrt((A11 - A22)^2 + 4 A12^2)) / (2 win^2)``, all float32.  If ``minEig < 1e-4`` or ``D < FLT_EPSILON`` the point
    is skipped at this level; at level 0 that sets ``status = 0``.

    Iteration, at most ``max_iter`` times.  The same bounds test runs on the moving window ``floor(next - half)``; failing it ends the level with ``next`` as it
    is, and at level 0 sets ``status = 0``.  ``b = 2^-20 sum (J - I) (Ix, Iy)`` with J sampled like I from the new image; ``delta = ((A12 b2 - A22 b1) * (1 / D),
    (A12 b1 - A11 b2) * (1 / D))``; ``next += delta``; stop when ``|delta|^2 <= eps^2`` (evaluated in float64).  From the second iteration on, if both components
    of ``delta + previous delta`` are below 0.01 in magnitude, step back by ``delta / 2`` and stop.

    After level 0 a point whose ``round(next - half)`` (half to even) lies outside the same bounds gets ``status = 0``.  A point with ``status = 0`` comes back as
    NaN (the reference overwrites lost points with NaN itself); a NaN input point is skipped and comes back NaN with status 0.

    Where this follows OpenCV's ``lkpyramid.cpp`` and not a plainer statement: ``delta`` multiplies by the float32 reciprocal ``1 / D`` and does not divide by
    ``D``; the bilinear fractions are taken from the float32 ``prev - half``; the stop test squares ``eps`` in float64.  Known NOT to follow it: OpenCV sums the
    window products in float32 (in an order that depends on its SIMD build) where this sums integers exactly, so results can differ in the last float32 bits.
    """
    if not (isinstance(win, (int, np.integer)) and win >= 1):
        raise ValueError(f"pyr_lk: win must be a positive integer, got {win!r}")
    pa = list(ref_pyramid) if ref_pyramid is not None else build_pyramid(ref_img, win, max_level)
    pb = list(new_pyramid) if new_pyramid is not None else build_pyramid(new_img, win, max_level)
    if len(pa) != len(pb) or any(a.shape != b.shape for a, b in zip(pa, pb)):
        raise ValueError("pyr_lk: the two images differ in size")
    pts = np.asarray(pts, dtype=np.float32).reshape(-1, 2)
    P = len(pts)
    live = ~np.isnan(pts).any(axis=1)
    base = np.where(live[:, None], pts, np.float32(0))
    status = live.copy()
    nxt = np.zeros((P, 2), dtype=np.float32)
    half = np.float32((win - 1) * 0.5)
    eps2 = float(eps) * float(eps)
    area2 = np.float32(2 * win * win)
    eig_log = np.full((P, len(pa)), np.nan, dtype=np.float32)
    margin = np.full(P, np.inf)
    with np.errstate(all="ignore"):
        for level in range(len(pa) - 1, -1, -1):
            I, J = pa[level], pb[level]
            h, w = I.shape
            prev = base * np.float32(1.0 / (1 << level))
            nxt = prev.copy() if level == len(pa) - 1 else nxt * np.float32(2)
            pw = prev - half
            ip = _to_int(np.floor(pw))
            out = _outside(ip[:, 0], ip[:, 1], w, h, win)
            margin[live] = np.minimum(margin[live], _margin(pw[live], w, h, win))
            if level == 0:
                status &= ~out
            idx = np.nonzero(live & ~out)[0]
            if idx.size == 0:
                continue
            gx, gy = scharr(I)
            ix, iy = ip[idx, 0], ip[idx, 1]
            wts = _weights(pw[idx, 0] - ix.astype(np.float32), pw[idx, 1] - iy.astype(np.float32))
            Iw = _blend(_patch(I, ix, iy, win, False), wts, _W_BITS - 5)
            Ix = _blend(_patch(gx, ix, iy, win, True), wts, _W_BITS)
            Iy = _blend(_patch(gy, ix, iy, win, True), wts, _W_BITS)
            A11 = (Ix * Ix).sum(axis=(1, 2)).astype(np.float32) * _FLT_SCALE
            A12 = (Ix * Iy).sum(axis=(1, 2)).astype(np.float32) * _FLT_SCALE
            A22 = (Iy * Iy).sum(axis=(1, 2)).astype(np.float32) * _FLT_SCALE
            D = A11 * A22 - A12 * A12
            dif = A11 - A22
            min_eig = (A22 + A11 - np.sqrt(dif * dif + np.float32(4) * A12 * A12)) / area2
            eig_log[idx, level] = min_eig
            weak = (min_eig.astype(np.float64) < _MIN_EIG) | (D < _FLT_EPSILON)
            if level == 0:
                status[idx[weak]] = False
            keep = ~weak
            idx, Iw, Ix, Iy, A11, A12, A22, D = idx[keep], Iw[keep], Ix[keep], Iy[keep], A11[keep], A12[keep], A22[keep], D[keep]
            Dinv = np.float32(1) / D
            nw = nxt[idx] - half  # the moving window's top-left, per running point
            pdelta = np.zeros((len(idx), 2), dtype=np.float32)
            run = np.arange(len(idx))  # positions in idx still iterating
            for j in range(max_iter):
                if run.size == 0:
                    break
                jp = _to_int(np.floor(nw[run]))
                out = _outside(jp[:, 0], jp[:, 1], w, h, win)
                margin[idx[run]] = np.minimum(margin[idx[run]], _margin(nw[run], w, h, win))
                if level == 0:
                    status[idx[run[out]]] = False
                run, jp = run[~out], jp[~out]
                if run.size == 0:
                    break
                jx, jy = jp[:, 0], jp[:, 1]
                wts = _weights(nw[run, 0] - jx.astype(np.float32), nw[run, 1] - jy.astype(np.float32))
                diff = _blend(_patch(J, jx, jy, win, False), wts, _W_BITS - 5) - Iw[run]
                b1 = (diff * Ix[run]).sum(axis=(1, 2)).astype(np.float32) * _FLT_SCALE
                b2 = (diff * Iy[run]).sum(axis=(1, 2)).astype(np.float32) * _FLT_SCALE
                delta = np.stack([(A12[run] * b2 - A22[run] * b1) * Dinv[run], (A12[run] * b1 - A11[run] * b2) * Dinv[run]], axis=1)
                nw[run] = nw[run] + delta
                nxt[idx[run]] = nw[run] + half
                d64 = delta.astype(np.float64)
                small = d64[:, 0] * d64[:, 0] + d64[:, 1] * d64[:, 1] <= eps2
                back = np.zeros(len(run), dtype=bool)
                if j > 0:
                    both = np.abs(delta + pdelta[run]).astype(np.float64)
                    back = ~small & (both[:, 0] < 0.01) & (both[:, 1] < 0.01)
                    nxt[idx[run[back]]] = nxt[idx[run[back]]] - delta[back] * np.float32(0.5)
                pdelta[run] = delta
                run = run[~(small | back)]
        last = _to_int(np.rint(nxt - half))
        margin[status] = np.minimum(margin[status], _margin((nxt - half)[status], pa[0].shape[1], pa[0].shape[0], win, rounded=True))
        status &= ~_outside(last[:, 0], last[:, 1], pa[0].shape[1], pa[0].shape[0], win)
    if info is not None:
        info["min_eig"], info["margin"] = eig_log, margin
    shifted = nxt.copy()
    shifted[~status] = np.nan
    return shifted, status.astype(np.uint8)


def as_gray_u8(image):
    """A frame as the reference's ``_preprocess_imgs`` leaves it for the flow: ``(H, W)``, ``(H, W, 1)`` or ``(1, H, W)``, a float frame truncated to uint8
    (``astype``).  Accepts arrays and tensors (a tensor stays where it is).  More than one channel is refused: the reference converts with ``cv2.cvtColor``."""
    import torch

    t = image if isinstance(image, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(image))
    if t.ndim == 3 and t.shape[-1] == 1:
        t = t[..., 0]
    elif t.ndim == 3 and t.shape[0] == 1:
        t = t[0]
    if t.ndim != 2:
        raise NotImplementedError(f"use_flow: frames with more than one channel are not built on the MI355X path (cv2.cvtColor), got a frame of shape {tuple(image.shape)}")
    if t.dtype != torch.uint8:
        t = t.to(torch.uint8)  # (truncation toward zero, as NumPy's astype)
    return t.contiguous()


# ---- the device path ------------------------------------------------------------------------------------------------

class JobDesc(C.Structure):
    """``ph_flow_job``."""

    _fields_ = [("ref", C.c_uint64 * MAX_LEVELS), ("cur", C.c_uint64 * MAX_LEVELS), ("pt_begin", C.c_int32), ("pt_end", C.c_int32)]


def pyramid_device(frames, win: int = 21, max_level: int = 3) -> List[List]:
    """``ph_flow_pyramid`` on the current stream: ``frames`` a uint8 device tensor (B, H, W); per frame the list of its level tensors, level 0 a view of
    ``frames`` and the levels above views of ONE new (B, S) tensor.  No host synchronisation."""
    import torch

    from sleap_nn_amd import _lib as L_

    L_.require_cuda(frames, "frames")
    if frames.dtype != torch.uint8 or frames.ndim != 3:
        raise ValueError(f"pyramid_device: a uint8 (B, H, W) tensor is needed, got {frames.dtype} {tuple(frames.shape)}")
    frames = frames.contiguous()
    B, H, W = (int(v) for v in frames.shape)
    sizes = (C.c_int32 * (2 * MAX_LEVELS))()
    n = L_.check(L_.lib().ph_flow_levels(H, W, int(win), int(max_level), C.cast(sizes, C.c_void_p)))
    shapes = [(sizes[2 * l], sizes[2 * l + 1]) for l in range(n)]
    S = sum(h * w for h, w in shapes[1:])
    with torch.cuda.device(frames.device):
        up = torch.empty((B, max(S, 1)), dtype=torch.uint8, device=frames.device)
        got = L_.check(L_.lib().ph_flow_pyramid(C.c_void_p(frames.data_ptr()), B, H, W, int(win), int(max_level), C.c_void_p(up.data_ptr()), B * S, L_.current_stream_ptr()))
    assert got == n
    out = []
    for b in range(B):
        levels, off = [frames[b]], 0
        for h, w in shapes[1:]:
            levels.append(up[b, off : off + h * w].view(h, w))
            off += h * w
        out.append(levels)
    return out


def track_device(jobs: Sequence[Tuple[Sequence, Sequence, np.ndarray]], win: int = 21, max_level: int = 3, max_iter: int = 30, eps: float = 0.01):
    """``ph_flow_track``, ONE launch for all ``jobs``: each ``(reference pyramid, current pyramid, points (P_j, 2))`` with the pyramids as ``pyramid_device`` gives
    them (same frame size, ``win`` and ``max_level`` throughout).  Returns per job ``(shifted (P_j, 2) float32 with NaN for lost points, status (P_j,) uint8)``,
    read back with one device-to-host copy."""
    import torch

    from sleap_nn_amd import _lib as L_

    lib = L_.lib()
    if lib.ph_flow_job_size() != C.sizeof(JobDesc):
        raise ImportError(f"struct ph_flow_job is {lib.ph_flow_job_size()} bytes, this binding's JobDesc {C.sizeof(JobDesc)}: rebuild the library")
    pts = [np.ascontiguousarray(p, dtype=np.float32).reshape(-1, 2) for _r, _c, p in jobs]
    total = sum(len(p) for p in pts)
    if not jobs or total == 0:
        return [(np.zeros((0, 2), np.float32), np.zeros(0, np.uint8)) for _ in jobs]
    level0 = jobs[0][0][0]
    L_.require_cuda(level0, "pyramid")
    dev, (H, W), n_levels = level0.device, (int(level0.shape[0]), int(level0.shape[1])), len(jobs[0][0])
    want = [(int(h), int(w)) for h, w in pyramid_shapes(H, W, int(win), int(max_level))] if MIN_WIN <= int(win) <= MAX_WIN and 0 <= int(max_level) < MAX_LEVELS else None
    if want is not None and [tuple(l.shape) for l in jobs[0][0]] != want:  # (the kernel reads the levels win and max_level name: they must be there)
        raise ValueError(f"track_device: the pyramids have levels {[tuple(l.shape) for l in jobs[0][0]]}, win={win} and max_level={max_level} need {want}")
    descs = (JobDesc * len(jobs))()
    begin = 0
    for d, (ref, cur, _p), p in zip(descs, jobs, pts):
        if [tuple(t.shape) for t in ref] != [tuple(t.shape) for t in jobs[0][0]] or [tuple(t.shape) for t in cur] != [tuple(t.shape) for t in jobs[0][0]]:
            raise ValueError("track_device: every pyramid of a launch must have the same frame size and levels")
        for l in range(n_levels):
            if ref[l].device != dev or cur[l].device != dev or not ref[l].is_contiguous() or not cur[l].is_contiguous() or ref[l].dtype != torch.uint8 or cur[l].dtype != torch.uint8:
                raise ValueError("track_device: pyramid levels must be dense uint8 tensors on one device")
            d.ref[l], d.cur[l] = ref[l].data_ptr(), cur[l].data_ptr()
        d.pt_begin, d.pt_end = begin, begin + len(p)
        begin += len(p)
    with torch.cuda.device(dev):
        jobs_dev = torch.frombuffer(bytearray(bytes(descs)), dtype=torch.uint8).to(dev)
        pts_dev = torch.from_numpy(np.concatenate(pts)).to(dev)
        rec = torch.empty(total * 9, dtype=torch.uint8, device=dev)  # [shifted float32 (P, 2) | status uint8 (P)]: one copy reads both
        L_.check(lib.ph_flow_track(C.c_void_p(jobs_dev.data_ptr()), len(jobs), max(len(p) for p in pts), C.c_void_p(pts_dev.data_ptr()), total, H, W, int(win), int(max_level),
                                   int(max_iter), float(eps), C.c_void_p(rec.data_ptr()), C.c_void_p(rec.data_ptr() + total * 8), L_.current_stream_ptr()))
        host = rec.cpu().numpy()
    shifted = host[: total * 8].view(np.float32).reshape(total, 2)
    status = host[total * 8 :]
    out, begin = [], 0
    for p in pts:
        out.append((shifted[begin : begin + len(p)].copy(), status[begin : begin + len(p)].copy()))
        begin += len(p)
    return out
