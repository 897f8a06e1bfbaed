"""Training augmentation on the GPU (ph_augment) against float64 NumPy restatements of the contract in
sleap_nn_amd/data/augmentation.py."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from sleap_nn_amd import _lib as L
from sleap_nn_amd.data import augmentation as A
from tests import _golden as G

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SIZES = [(97, 130), (384, 384), (1024, 1024)]


def _frames(B, Cc, hw, seed=0, dtype=torch.uint8):
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(0, 256, (B, Cc, hw[0], hw[1]), dtype=torch.uint8, generator=g)
    return x.to(DEV) if dtype == torch.uint8 else (x.float() / 255.0).to(DEV)


def _kps(B, I, N, hw, seed=0):
    g = np.random.RandomState(seed)
    k = (g.rand(B, I, N, 2) * [hw[1] - 1, hw[0] - 1]).astype(np.float32)
    k[:, 0, 1] = np.nan
    return torch.from_numpy(k).to(DEV)


def _run(img, kp, draws, sym=(), icfg=None, seed=0, counters=None):
    H, W = img.shape[-2:]
    return A._launch(img, kp, A._pack(draws, H, W, icfg, seed), sym, counters)


def _affine(angle, s, tx, ty, hw):
    cx, cy = hw[1] / 2, hw[0] / 2
    m = A._concat(A._rotate(angle, cx, cy), A._scale(s, s, cx, cy))
    return A._concat(m, A._translate(tx, ty))


# ---------------------------------------------------------------------------------------------------------------------
# float64 restatement of the warp
# ---------------------------------------------------------------------------------------------------------------------
def _edges64(m, h, w):
    corners = [(m[0] * x + m[1] * y + m[2], m[3] * x + m[4] * y + m[5]) for x, y in ((0, 0), (w, 0), (w, h), (0, h))]
    ctr = np.mean(corners, axis=0)
    out = []
    for k in range(4):
        (x0, y0), (x1, y1) = corners[k], corners[(k + 1) % 4]
        nx, ny = -(y1 - y0), x1 - x0
        nn = math.hypot(nx, ny)
        nx, ny = nx / nn, ny / nn
        d = -(nx * x0 + ny * y0)
        if nx * ctr[0] + ny * ctr[1] + d < 0:
            nx, ny, d = -nx, -ny, -d
        out.append((nx, ny, d))
    return out


def _clip_area(px, py, edges):
    poly = [(px, py), (px + 1, py), (px + 1, py + 1), (px, py + 1)]
    for nx, ny, d in edges:
        res = []
        for i in range(len(poly)):
            a, b = poly[i], poly[(i + 1) % len(poly)]
            da, db = nx * a[0] + ny * a[1] + d, nx * b[0] + ny * b[1] + d
            if da >= 0:
                res.append(a)
            if (da >= 0) != (db >= 0):
                t = da / (da - db)
                res.append((a[0] + t * (b[0] - a[0]), a[1] + t * (b[1] - a[1])))
        poly = res
        if len(poly) < 3:
            return 0.0
    return 0.5 * abs(sum(poly[i][0] * poly[(i + 1) % len(poly)][1] - poly[(i + 1) % len(poly)][0] * poly[i][1] for i in range(len(poly))))


def _ref_warp(src, m32, flip):
    """src (C, H, W) uint8 -> (value before rounding, coverage, class) with class 0 outside, 1 edge, 2 interior."""
    Cc, H, W = src.shape
    m = m32.astype(np.float64)
    Ai = np.linalg.inv(np.array([[m[0], m[1]], [m[3], m[4]]]))
    t = -Ai @ np.array([m[2], m[5]])
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float64)
    px, py = xs + 0.5, ys + 0.5
    qx = Ai[0, 0] * px + Ai[0, 1] * py + t[0]
    qy = Ai[1, 0] * px + Ai[1, 1] * py + t[1]
    if flip:
        qx = W - qx
    u, v = qx - 0.5, qy - 0.5
    x0, y0 = np.floor(u), np.floor(v)
    fx, fy = u - x0, v - y0
    xa, xb = np.clip(x0, 0, W - 1).astype(int), np.clip(x0 + 1, 0, W - 1).astype(int)
    ya, yb = np.clip(y0, 0, H - 1).astype(int), np.clip(y0 + 1, 0, H - 1).astype(int)
    s = src.astype(np.float64)
    val = (s[:, ya, xa] * (1 - fx) + s[:, ya, xb] * fx) * (1 - fy) + (s[:, yb, xa] * (1 - fx) + s[:, yb, xb] * fx) * fy
    edges = _edges64(m, H, W)
    cls = np.full((H, W), 2, np.int8)
    partial = np.zeros((H, W), bool)
    for nx, ny, d in edges:
        dist = nx * px + ny * py + d
        half = 0.5 * (abs(nx) + abs(ny))
        cls[dist <= -half - 1e-3] = 0
        partial |= np.abs(dist) < half + 1e-3
    cov = np.where(cls == 0, 0.0, 1.0)
    edge = partial & (cls != 0)
    cls[edge] = 1
    for y, x in zip(*np.nonzero(edge)):
        cov[y, x] = _clip_area(float(x), float(y), edges)
    return val * cov, cov, cls


def _check_warp(out, src, m32, flip, lsb=1.0):
    want, cov, cls = _ref_warp(src, m32, flip)
    got = out.astype(np.float64)
    inner = np.broadcast_to(cls == 2, got.shape)
    w_in = want[inner]
    d_in = np.abs(got[inner] - np.floor(w_in + 0.5))
    # a value within 0.01 of a rounding tie may round either way under the kernel's fp32 coordinates: it counts against
    # the 1-LSB bound but not against the share of exact pixels
    tie = np.abs(w_in - np.floor(w_in) - 0.5) < 0.01
    assert d_in.size == 0 or (d_in.max() <= lsb and (d_in[~tie] == 0).mean() >= 0.995), (d_in.max(), (d_in[~tie] == 0).mean())
    e = np.broadcast_to(cls == 1, got.shape)
    d_e = np.abs(got[e] - want[e])
    assert d_e.size == 0 or d_e.max() <= 2.0 * lsb, d_e.max()
    o = np.broadcast_to(cls == 0, got.shape)
    assert (got[o] == 0).all()
    return int(inner.sum()), int(e.sum()), int(o.sum())


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw", SIZES)
@pytest.mark.parametrize("Cc", [1, 3])
@pytest.mark.parametrize("B", [1, 4, 32])
def test_identity_and_flip_are_exact(B, Cc, hw):
    img = _frames(B, Cc, hw, seed=B + Cc)
    kp = _kps(B, 2, 5, hw, seed=B)
    out, k = _run(img, kp, [A.SampleDraw() for _ in range(B)])
    assert torch.equal(out, img) and out.data_ptr() != img.data_ptr()
    assert torch.equal(torch.isnan(k), torch.isnan(kp)) and torch.equal(torch.nan_to_num(k), torch.nan_to_num(kp))
    sym = [(0, 3), (1, 2)]
    flips = [A.SampleDraw(flip=bool(i % 2 == 0)) for i in range(B)]
    out, k = _run(img, kp, flips, sym)
    want = kp.clone()
    want[..., 0] = (hw[1] - 1) - want[..., 0]
    for a, b in sym:
        want[..., [a, b], :] = want[..., [b, a], :]
    for i in range(B):
        if i % 2 == 0:
            assert torch.equal(out[i], torch.flip(img[i], dims=[-1]))
            assert torch.equal(torch.isnan(k[i]), torch.isnan(want[i])) and torch.equal(torch.nan_to_num(k[i]), torch.nan_to_num(want[i]))
        else:
            assert torch.equal(out[i], img[i]) and torch.equal(torch.nan_to_num(k[i]), torch.nan_to_num(kp[i]))


def _lut(c, b):
    v = np.arange(256, dtype=np.float32)
    lut = v.astype(np.uint8)
    if c is not None:
        lut = np.clip((v - np.float32(127.5)) * np.float32(c) + np.float32(127.5), 0, 255).astype(np.uint8)
    if b is not None:
        lut = np.clip(lut.astype(np.float32) * np.float32(b), 0, 255).astype(np.uint8)
    return lut


@pytest.mark.parametrize("Cc", [1, 3])
def test_contrast_brightness_match_the_lut_and_the_reference(Cc):
    rng = np.random.RandomState(3)
    B, hw = 6, (97, 130)
    img = _frames(B, Cc, hw, seed=5)
    draws = [A.SampleDraw(contrast=float(rng.uniform(0.3, 2.5)) if i != 1 else None, brightness=float(rng.uniform(0.2, 1.9)) if i != 2 else None) for i in range(B)]
    out, _ = _run(img, None, draws)
    x = img.cpu().numpy()
    for i, d in enumerate(draws):
        assert np.array_equal(out[i].cpu().numpy(), _lut(d.contrast, d.brightness)[x[i]]), i
    z = G.load("augment_draws.npz")
    for i in range(4):
        src = torch.from_numpy(z[f"intensity/{i}/input"]).to(DEV)
        b = float(z[f"intensity/{i}/brightness"])
        d = A.SampleDraw(contrast=float(z[f"intensity/{i}/contrast"]), brightness=None if np.isnan(b) else b)
        got, _ = _run(src, None, [d])
        assert np.array_equal(got.cpu().numpy(), z[f"intensity/{i}/output"]), i


def test_noise():
    B, hw = 4, (512, 512)
    base = torch.full((B, 1) + hw, 100, dtype=torch.uint8, device=DEV)
    # degenerate cases are exact
    cfg = dict(A.INTENSITY_DEFAULTS, uniform_noise_min=0.1, uniform_noise_max=0.1, gaussian_noise_mean=0.05, gaussian_noise_std=0.0)
    out, _ = _run(base, None, [A.SampleDraw(uniform=True)] * B, icfg=cfg, seed=11)
    assert (out == 100 + 25).all()
    out, _ = _run(base, None, [A.SampleDraw(gaussian=True)] * B, icfg=cfg, seed=11)
    assert (out == 100 + 12).all()  # trunc(0.05 * 255)
    # uniform: every value of [lo, hi] inclusive, frequencies within 5 sigma
    cfg = dict(A.INTENSITY_DEFAULTS, uniform_noise_min=0.0, uniform_noise_max=0.04)
    out, _ = _run(base, None, [A.SampleDraw(uniform=True)] * B, icfg=cfg, seed=12)
    n = (out.to(torch.int64) - 100).flatten()
    assert int(n.min()) == 0 and int(n.max()) == 10
    cnt = torch.bincount(n, minlength=11).cpu().numpy().astype(np.float64)
    p = 1.0 / 11
    assert np.all(np.abs(cnt - n.numel() * p) <= 5 * math.sqrt(n.numel() * p * (1 - p))), cnt
    # Gaussian: mean and std of trunc(N(0, 25.5)) on ~1 M pixels
    cfg = dict(A.INTENSITY_DEFAULTS, gaussian_noise_mean=0.0, gaussian_noise_std=0.1)
    base2 = torch.full((B, 1) + hw, 128, dtype=torch.uint8, device=DEV)
    out, _ = _run(base2, None, [A.SampleDraw(gaussian=True)] * B, icfg=cfg, seed=13)
    g = (out.to(torch.float64) - 128).flatten().cpu().numpy()
    ref = np.trunc(np.random.RandomState(0).normal(0, 25.5, g.size))
    sd = ref.std()
    assert abs(g.mean() - ref.mean()) <= 5 * sd * math.sqrt(2.0 / g.size), (g.mean(), ref.mean())
    assert abs(g.std() / sd - 1) <= 0.01, (g.std(), sd)
    # same seed -> same bytes; other sample / other seed -> other noise
    cfg = dict(A.INTENSITY_DEFAULTS, uniform_noise_min=0.0, uniform_noise_max=0.2, gaussian_noise_std=0.05)
    d = [A.SampleDraw(uniform=True, gaussian=True)] * B
    a1, _ = _run(base2, None, d, icfg=cfg, seed=21)
    a2, _ = _run(base2, None, d, icfg=cfg, seed=21)
    a3, _ = _run(base2, None, d, icfg=cfg, seed=22)
    assert torch.equal(a1, a2)
    assert not torch.equal(a1[0], a1[1]) and not torch.equal(a1, a3)
    assert (a1[0] != a3[0]).float().mean() > 0.5


WARPS = [(180.0, 1.0, 0.0, 0.0, False), (-180.0, 0.9, 3.0, -2.0, True), (37.0, 1.5, 10.5, 4.25, False), (-63.0, 0.25, -5.0, 7.0, True), (90.0, 0.5, 0.0, 0.0, False),
         (12.0, 1.1, -20.0, 15.0, True), (0.0, 0.25, 0.0, 0.0, False), (-135.0, 1.3, 0.0, 0.0, False)]


@pytest.mark.parametrize("hw,B,Cc,check", [((97, 130), 8, 1, range(8)), ((97, 130), 8, 3, range(8)), ((384, 384), 8, 1, range(8)), ((384, 384), 32, 3, (0, 3, 5)),
                                           ((1024, 1024), 8, 1, (0, 3)), ((1024, 1024), 32, 1, (1, 7, 30))])
def test_warp_matches_the_restatement(hw, B, Cc, check):
    img = _frames(B, Cc, hw, seed=hw[0] + B)
    draws = []
    for i in range(B):
        ang, s, tx, ty, fl = WARPS[i % len(WARPS)]
        draws.append(A.SampleDraw(warp=True, flip=fl, matrix=_affine(ang, s, tx, ty, hw)))
    cnt = torch.zeros(4, dtype=torch.int32, device=DEV)
    out, _ = _run(img, None, draws, counters=cnt)
    c = cnt.cpu().numpy()
    assert c[0] == 0 and c[2] > 0, c
    if hw[0] * hw[1] > 20480:  # the frame is larger than one staged box: scale 0.25 takes the direct-gather path
        assert c[3] > 0, c
    src, got = img.cpu().numpy(), out.cpu().numpy()
    totals = np.zeros(3, np.int64)
    for i in check:
        totals += _check_warp(got[i], src[i], draws[i].matrix, draws[i].flip)
    assert totals.min() > 0  # interior, edge and outside pixels all checked


def test_warp_float_frames_within_one_level():
    hw, B = (97, 130), 8
    img = _frames(B, 3, hw, seed=4, dtype=torch.float32)
    draws = [A.SampleDraw(warp=True, flip=w[4], matrix=_affine(*w[:4], hw)) for w in WARPS]
    out, _ = _run(img, None, draws)
    q = (img.cpu().numpy() * np.float32(255)).astype(np.uint8)
    got = out.cpu().numpy() * 255.0
    for i in range(B):
        _check_warp(got[i], q[i], draws[i].matrix, draws[i].flip, lsb=1.0 + 1e-3)
    out_u8, _ = _run(torch.from_numpy(q).to(DEV), None, draws)
    assert np.abs(out.cpu().numpy() - out_u8.cpu().numpy() / 255.0).max() <= 1e-6


def test_device_keypoints_follow_the_matrix():
    hw, B = (384, 384), 8
    kp = _kps(B, 3, 6, hw, seed=9)
    sym = [(0, 5), (2, 3)]
    draws = [A.SampleDraw(warp=True, flip=w[4], matrix=_affine(*w[:4], hw)) for w in WARPS]
    _, k = _run(_frames(B, 1, hw), kp, draws, sym)
    src = kp.cpu().numpy().astype(np.float64)
    got = k.cpu().numpy()
    for i, d in enumerate(draws):
        p = src[i].copy()
        if d.flip:
            p[..., 0] = (hw[1] - 1) - p[..., 0]
            for a, b in sym:
                p[..., [a, b], :] = p[..., [b, a], :]
        m = d.matrix.astype(np.float64)
        want = np.stack([m[0] * p[..., 0] + m[1] * p[..., 1] + m[2], m[3] * p[..., 0] + m[4] * p[..., 1] + m[5]], -1)
        assert np.array_equal(np.isnan(got[i]), np.isnan(want))
        assert np.nanmax(np.abs(got[i] - want)) <= 1e-3


def test_fused_equals_separate_calls():
    hw, B = (384, 384), 6
    img = _frames(B, 3, hw, seed=8)
    kp = _kps(B, 2, 4, hw, seed=8)
    icfg = dict(A.INTENSITY_DEFAULTS, uniform_noise_min=0.0, uniform_noise_max=0.1, gaussian_noise_std=0.03)
    rng = np.random.RandomState(5)
    fused, inten, geo = [], [], []
    for i in range(B):
        ang, s, tx, ty, fl = WARPS[i]
        er = (int(rng.randint(0, 300)), int(rng.randint(0, 300)), 40, 60)
        fill = rng.randint(0, 256, 3).astype(np.uint8)
        kw = dict(uniform=True, gaussian=i % 2 == 0)
        cb = dict(contrast=float(rng.uniform(0.5, 1.5)), brightness=float(rng.uniform(0.5, 1.5)))
        gw = dict(warp=i != 2, flip=fl, matrix=_affine(ang, s, tx, ty, hw), erase=er, fill=fill)
        fused.append(A.SampleDraw(**kw, **cb, **gw))
        inten.append(A.SampleDraw(**kw, **cb))
        geo.append(A.SampleDraw(**gw))
    sym = [(0, 1)]
    a, ka = _run(img, kp, fused, sym, icfg=icfg, seed=77)
    mid, _ = _run(img, None, inten, icfg=icfg, seed=77)
    b, kb = _run(mid, kp, geo, sym)
    assert torch.equal(a, b)
    assert torch.equal(torch.isnan(ka), torch.isnan(kb)) and torch.equal(torch.nan_to_num(ka), torch.nan_to_num(kb))
    # the erase rectangle holds its fill
    for i, d in enumerate(fused):
        y, x, eh, ew = d.erase
        for c in range(3):
            assert (a[i, c, y : y + eh, x : x + ew] == int(d.fill[c])).all()


def _dots(B, hw, kp):
    img = np.zeros((B, 1) + hw, np.uint8)
    k = kp.cpu().numpy()
    for b in range(B):
        for p in k[b].reshape(-1, 2):
            if np.isnan(p).any():
                continue
            x, y = int(round(float(p[0]))), int(round(float(p[1])))
            img[b, 0, y - 1 : y + 2, x - 1 : x + 2] = 255
    return torch.from_numpy(img).to(DEV)


def test_dots_follow_their_keypoints():
    """Bright 3x3 dots drawn at the keypoints land where the augmented keypoints say, up to the reference's own half-pixel
    offset between the image (pixel centres) and the keypoints (raw coordinates)."""
    hw, B = (192, 256), 8
    g = np.random.RandomState(2)
    k = np.round(np.stack([g.uniform(110, 146, (B, 2, 4)), g.uniform(80, 112, (B, 2, 4))], -1)).astype(np.float32)
    for b in range(B):  # keep the dots of a sample apart
        k[b] = k[b, 0, 0] + np.array([[[0, 0], [14, 0], [0, 14], [14, 14]], [[-14, 0], [-14, 14], [-14, -14], [0, -14]]], np.float32)
    kp = torch.from_numpy(k).to(DEV)
    img = _dots(B, hw, kp)
    aug = A.Augmenter(None, dict(rotation_min=-180.0, rotation_max=180.0, scale_min=0.8, scale_max=1.2, flip_p=0.5), symmetric_inds=[(0, 1), (2, 3)],
                      rng=np.random.RandomState(4))
    state = aug.rng.get_state()
    out, ka = aug(img, kp)
    aug.rng.set_state(state)
    draws, _ = aug.draw(B, hw)
    o, kk = out.cpu().numpy().astype(np.float64), ka.cpu().numpy()
    worst_centre = worst_raw = 0.0
    for b in range(B):
        m = draws[b].matrix.astype(np.float64)
        L_ = np.array([[m[0], m[1]], [m[3], m[4]]])
        for p in kk[b].reshape(-1, 2):
            cx, cy = int(round(p[0])), int(round(p[1]))
            win = o[b, 0, cy - 5 : cy + 6, cx - 5 : cx + 6]
            ys, xs = np.mgrid[cy - 5 : cy + 6, cx - 5 : cx + 6]
            c = np.array([(win * xs).sum(), (win * ys).sum()]) / win.sum()
            centre = p + L_ @ np.array([0.5, 0.5]) - 0.5  # where pixel (i, j) of the source (centre i+0.5, j+0.5) lands, as an index
            worst_centre = max(worst_centre, float(np.hypot(*(c - centre))))
            worst_raw = max(worst_raw, float(np.hypot(*(c - p))))
    assert worst_centre <= 1.0, worst_centre
    assert worst_raw <= 1.0 + math.sqrt(2) * 0.5 * 1.2 + 1e-6, worst_raw  # |L (0.5, 0.5) - (0.5, 0.5)| <= 0.707 (s + 1)


def test_augmented_batch_trains():
    from oracle import cpu_ref as O
    from sleap_nn_amd.architectures.model import Model
    from sleap_nn_amd.data.targets import generate_multiconfmaps, generate_pafs
    from sleap_nn_amd.training.module import TrainingModule

    bb = {"in_channels": 1, "kernel_size": 3, "filters": 8, "filters_rate": 2, "max_stride": 8, "stem_stride": None, "middle_block": True,
          "up_interpolate": True, "stacks": 1, "convs_per_block": 2, "output_stride": 2}
    names = ["n0", "n1", "n2"]
    heads = {"confmaps": {"part_names": names, "output_stride": 2, "loss_weight": 1.0},
             "pafs": {"edges": [["n0", "n1"], ["n1", "n2"]], "output_stride": 4, "loss_weight": 1.0}}
    sd = O.init_state(bb, heads, "bottomup", seed=3, head_scale=1.0)
    m = Model("unet", bb, heads, "bottomup")
    m.load_state_dict(sd)
    tm = TrainingModule(m, DEV, lr=1e-3)
    hw, B = (64, 96), 4
    g = np.random.RandomState(1)
    k = np.stack([g.uniform(25, 70, (B, 2, 3)), g.uniform(18, 46, (B, 2, 3))], -1).astype(np.float32)
    kp = torch.from_numpy(k).to(DEV)
    aug = A.Augmenter(dict(contrast_p=0.5, brightness_p=0.5), dict(rotation_min=-180.0, rotation_max=180.0, flip_p=0.5, erase_p=0.5),
                      symmetric_inds=[(0, 2)], rng=np.random.RandomState(0))
    img, ka = aug(_dots(B, hw, kp), kp)
    batch = {"image": img, "MultiInstanceConfmapsHead": generate_multiconfmaps(ka, hw, sigma=1.5, output_stride=2),
             "PartAffinityFieldsHead": generate_pafs(ka, hw, sigma=1.5, output_stride=4, edge_inds=[(0, 1), (1, 2)])}
    losses = [float(tm.training_step(batch)[0]) for _ in range(6)]
    tm.close()
    assert all(math.isfinite(v) for v in losses) and losses[-1] < losses[0], losses


def test_bad_arguments_return_errors():
    lib = L.lib()
    img = torch.zeros((2, 1, 16, 16), dtype=torch.uint8, device=DEV)
    out = torch.empty_like(img)
    par = torch.zeros(2 * C.sizeof(L.AugSample), dtype=torch.uint8, device=DEV)
    s = L.current_stream_ptr()
    P = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    assert lib.ph_augment(None, P(out), 0, 2, 1, 16, 16, None, None, 0, 0, P(par), None, 0, None, s) == L.PH_E_INVALID
    assert lib.ph_augment(P(img), P(out), 0, 2, 2, 16, 16, None, None, 0, 0, P(par), None, 0, None, s) == L.PH_E_INVALID
    assert lib.ph_augment(P(img), P(out), 7, 2, 1, 16, 16, None, None, 0, 0, P(par), None, 0, None, s) == L.PH_E_INVALID
    assert lib.ph_augment(P(img), P(img), 0, 2, 1, 16, 16, None, None, 0, 0, P(par), None, 0, None, s) == L.PH_E_INVALID
    assert lib.ph_augment(P(img), P(out), 0, 2, 1, 16, 16, P(par), None, 0, 0, P(par), None, 0, None, s) == L.PH_E_INVALID
    kp = torch.zeros((2, 1, 3, 2), device=DEV)
    assert lib.ph_augment(P(img), P(out), 0, 2, 1, 16, 16, P(kp), P(kp), 1, 3, P(par), None, 0, None, s) == L.PH_E_INVALID
    assert lib.ph_augment(P(img), P(out), 0, 2, 1, 16, 16, P(kp), P(torch.empty_like(kp)), 1, 3, P(par), None, 1, None, s) == L.PH_E_INVALID
    assert "overlap" in lib.ph_last_error().decode() or "pair" in lib.ph_last_error().decode()
    with pytest.raises(ValueError, match="channels"):
        A.Augmenter()(torch.zeros((1, 2, 8, 8), dtype=torch.uint8, device=DEV))
