"""Reference, operands and case table of the exact-fp32 3x3 conv tests (the eight kernels behind ``conv3x3_route``, csrc/conv3x3_route.h; DESIGN.md 4.1, "Held to float64 at the
tile edges"), shared by tests/test_conv3x3_cpu.py and tests/test_gpu_conv3x3.py.  Every case is ONE launch through ``ph_debug_conv3x3_run`` on tensors the test owns.

Reference: float64, plain torch, NCHW tensors of the TRUE channel counts.  A half-resolution second source goes through ``F.interpolate(scale_factor=2, mode="bilinear",
align_corners=False)``, then the concat, ``F.conv2d(padding=1)`` and the epilogue as ``ConvArgs`` (csrc/net_kernels.h) documents it:

    y = conv + bias;  relu;  (accumulate) y += old dst;  (relu_mask_src) y = mask > 0 ? y : 0;
    dst_pool = 2x2/2 max pool of y at ceil(H/2) x ceil(W/2), elements beyond the image counting as 0 (the kernels' "same" padding; every pool case runs with relu = 1,
               where that is the plain ceil-mode pool);
    head_dst[b][o][y][x] = (sigmoid)(sum_c head_w[o][c] y[c] + head_b[o]), NCHW.

Pad channels of dst (true cout up to pad16(cout)): every kernel writes them, with the packers' zero weight rows and zero bias, so they are the epilogue of 0 -- 0, or the old
value under ``accumulate`` (then masked like any other channel).  The reference states that by zero-padding weight and bias to pad16(cout), and the tests pin it.

Beside each value the reference returns S = sum |x||w| + |bias| (+ |old dst|), the magnitude sum the direct kernels' bound is built on.

Two operand families:
  exact   small integers (sources in [-4, 4]; weights in [-4, 4], multiples of 4 in [-8, 8] where the kernel is F(2,3) or F(2x2,3x3), whose G only halves; a
          half-resolution source in multiples of 16, so that the interpolation weights 1/16 .. 9/16 leave integers).  Every partial sum in any order is an fp32 integer while
          the magnitude sum THROUGH the transforms, |A^T| [sum_c (|G||g||G^T|) * (|B^T||d||B|)] |A|, stays below 2^24 (test_conv3x3_cpu.py asserts it for every exact case),
          so the three direct kernels and the four F(2,3) / F(2x2,3x3) kernels must come out EQUAL to the reference, pool and head included.
          F(4x4,3x3) is exempt from equality: its device weight transform (wino4_g_row) multiplies by fp32 1/6, 1/12, 1/24 and may contract into FMAs, so a cancelling
          sum need not be exact.  Its exact-family launches are held to the rigorous bound below (and serve the guards).
  float   uniform in [-0.5, 0.5).
          Direct kernels (register-staged, 9-tap, conv3x3_c16): per element |d - r| <= gamma_n S, n = 9 K + 3, gamma_n = n u / (1 - n u), u = 2^-24.
          Winograd kernels: the rigorous bound is gamma_n times the magnitude sum through the transforms (n = K + WINO_ROUNDINGS); it is the outer limit, not the bar.
          The bar is 4 e32, where e32 = max |fp32 - float64| of the reference's OWN float32 evaluation of the same algorithm with the textbook matrices (``winograd``,
          the fold included), and never above the rigorous bound.  The factor four leaves room for another summation order (MFMA blocks of four, K slices).
          e32 per case comes from the reference alone: ``MEASURED`` below, written by test_conv3x3_cpu.py's recorder (CONV3X3_RECORD=1) at the geometry of a 256-CU chip;
          on a chip with another CU count the cases whose map depends on it recompute theirs.
          Fused head: the pre-activation's bar is the conv's bar times sum |head_w| plus gamma_(coutp + 2) times its own magnitude sum.  A sigmoid head runs a second
          launch without the sigmoid: the pre-activations must be bitwise equal, and the device sigmoid of its own argument is held to ``SIGMOID_BAR`` u.

Out of scope: the 4 GiB offset guards (wino2d_fits, w16_fits, wino4_shape_ok) need tensors no test should allocate; splitk_finish = 2 (workgroups wait for each other) stays
covered by tests/test_gpu_small_batch.py alone.
"""
from __future__ import annotations

from dataclasses import dataclass, field, replace
from typing import Callable, Optional, Union

import torch
import torch.nn.functional as F

from tests._conv_routes import (A_ACCUMULATE, A_HEAD, A_LOWRES, A_POOL, A_RELU_MASK, A_SKIP_DST, A_SRC1, F_C16, F_DMA, F_SM, F_W16, F_WINO, F_WINO2, F_WINO4, K_C16, K_DMA9,
                                K_REGSTAGED, K_SMALLMAP, K_W16, K_WINO1D, K_WINO2D, K_WINO4, KERNEL_NAMES, P_HEAD_SM, P_HEAD_W16, P_HEAD_W2D, P_LOWRES, P_MASK, P_POOLS, w16_shape_ok)

U = 2.0 ** -24
NAN = float("nan")
CHIP_CUS = 256     # an MI355X; the CPU tests ask the route with it, the persistent grids themselves are sized by the device's own count


def guard_pixels(W: int) -> int:
    """NaN pixels before and after every device tensor: more than one map row + 1, so that a tap one row outside the first or last image lands in them."""
    return W + 8

WINO_ROUNDINGS = 40  # roundings of one output besides its K products' sum: G g G^T (<= 8), B^T d B (<= 12), A^T M A (<= 12), K slices, bias, the bilinear fold (<= 4)
TILE = {K_REGSTAGED: (8, 32), K_DMA9: (16, 32), K_WINO1D: (16, 32), K_C16: (8, 32), K_W16: (32, 16), K_WINO2D: (16, 16), K_WINO4: (16, 32), K_SMALLMAP: (8, 8)}  # (rows, columns)
DIRECT = (K_REGSTAGED, K_DMA9, K_C16)
WINO_M = {K_WINO1D: (2, False), K_W16: (2, True), K_WINO2D: (2, True), K_SMALLMAP: (2, True), K_WINO4: (4, True)}  # output tile size, two-dimensional
PERSISTENT = (K_DMA9, K_WINO1D, K_C16, K_W16, K_WINO2D, K_WINO4)

# |sigmoid_device(x) - sigmoid(x)| <= c u for the fused heads' 1 / (1 + expf(-x)): c = twice the worst value an MI355X gave over the sigmoid cases of the table (the margin
# tests/_row_gemm.py gives ACT_BAR), measured against the float64 sigmoid of the device's own pre-activation.  csrc/device_math.h states no error for it.
SIGMOID_MEASURED = 1.4500
SIGMOID_BAR = None if SIGMOID_MEASURED is None else 2.0 * SIGMOID_MEASURED

STEER = {  # the option fields that bring a launch to each kernel, as the product's handle options would
    K_REGSTAGED: dict(use_dma=0),
    K_DMA9: dict(use_wino=0, use_c16=0),
    K_WINO1D: dict(use_w16=0, use_wino2d=0, use_c16=0),
    K_C16: dict(use_w16=0),  # (16 -> 16 channels are a shape of the wave-private kernel first)
    K_W16: dict(),
    K_WINO2D: dict(),
    K_WINO4: dict(use_wino4=2),
    K_SMALLMAP: dict(use_sm=2),
}
BASE_OPTIONS = dict(use_dma=1, dma32=1, use_wino=1, persist=1, use_c16=1, use_w16=1, use_wino2d=1, use_wino4=0, wino4_min_cin=64, use_sm=0, splitk=0)

# every (kernel, instantiation) pair launch_conv3x3_routed and the four launchers (launch_conv3x3_w16, launch_conv3x3_wino2d, launch_conv3x3_wino4, launch_conv3x3_sm) can
# dispatch, written out from their code
PAIRS = (
    [(K_REGSTAGED, "bn64"), (K_REGSTAGED, "bn32")]                                                            # launch_conv3x3: conv3x3_mfma_kernel<64 | 32>
    + [(K_DMA9, "persist_bn64"), (K_DMA9, "persist_bn32"), (K_DMA9, "tile_bn64"), (K_DMA9, "tile_bn32")]      # conv3x3_mfma_dma_persist_kernel / conv3x3_mfma_dma_kernel
    + [(K_WINO1D, "bn64"), (K_WINO1D, "bn32")]                                                                # conv3x3_wino_persist_kernel<64 | 32, 8>
    + [(K_C16, "")]
    + [(K_W16, i) for i in ("1,1,head", "2,2,head", "1,1", "2,1", "1,2", "2,2", "2,1,two", "3,1,two", "4,1,two", "2,2,two")]  # conv3x3_w16_kernel<CHUNKS, NB, TWO, HEAD>
    + [(K_WINO2D, i) for i in ("plain", "ht", "bwd", "ht_bwd", "ks")]                                         # conv3x3_wino2d_kernel<64, HT, BWD, KS>
    + [(K_WINO4, i) for i in ("plain", "lowres", "ks", "lowres_ks")]                                          # conv3x3_wino4_kernel<LOWRES, KS>
    + [(K_SMALLMAP, i) for i in ("false,1", "false,2", "true,1", "true,2")]                                   # conv3x3_sm_kernel<LOWRES, NB>
)


def pad16(c: int) -> int:
    return (c + 15) // 16 * 16


def gamma(n: int) -> float:
    return n * U / (1.0 - n * U)


@dataclass(frozen=True)
class Case:
    name: str
    kernel: int                              # the kernel the case is there for (asserted from the route's report)
    cout: int
    cin0: int
    cin1: int = 0
    H: Union[int, Callable[[int], int]] = 16
    W: Union[int, Callable[[int], int]] = 32
    B: int = 3
    bn: int = 0                              # 0: the product's choice (64 from 64 padded output channels on); 64 with 32 padded output channels: the half-empty-tile packing
    relu: int = 1
    accumulate: bool = False
    mask: bool = False
    pool: bool = False
    skip_dst: bool = False
    lowres: bool = False
    head: int = 0                            # head channels (0: no fused head)
    sigmoid: bool = False
    splitk: int = 0
    scratch: Optional[str] = None            # None: no split scratch; "fits": ksplit planes and one spare; "short": one byte less than ksplit planes (-> one stage)
    splitk_finish: int = 0
    ksplit: int = 1                          # the K slices the route must report
    opts: tuple = ()                         # option fields over STEER[kernel]
    tags: tuple = field(default_factory=tuple)

    @property
    def direct(self) -> bool:
        return self.kernel in DIRECT


def geometry(c: Case, n_cu: int = CHIP_CUS) -> dict:
    H = c.H(n_cu) if callable(c.H) else c.H
    W = c.W(n_cu) if callable(c.W) else c.W
    coutp, c0p, c1p = pad16(c.cout), pad16(c.cin0), pad16(c.cin1) if c.cin1 else 0
    bn = c.bn or (64 if coutp >= 64 else 32)
    th, tw = TILE[c.kernel]
    tiles = c.B * ((H + th - 1) // th) * ((W + tw - 1) // tw)
    ntc = (coutp + bn - 1) // bn if c.kernel in (K_REGSTAGED, K_DMA9, K_WINO1D) else ((coutp + 63) // 64 if c.kernel in (K_WINO2D, K_WINO4) else 1)
    forms = F_WINO | F_SM | (0 if (bn == 64 and coutp == 32) else F_DMA)
    if bn == 64:
        forms |= F_WINO2 | (F_WINO4 if c0p + c1p >= 64 else 0)
    if bn == 32 and w16_shape_ok(c0p, c1p, coutp):
        forms |= F_W16
    if c.cin1 == 0 and c.cin0 <= 16 and c.cout <= 16:
        forms |= F_C16
    flags = ((A_SRC1 if c.cin1 else 0) | (A_LOWRES if c.lowres else 0) | (A_POOL if c.pool else 0) | (A_SKIP_DST if c.skip_dst else 0) | (A_ACCUMULATE if c.accumulate else 0)
             | (A_RELU_MASK if c.mask else 0) | (A_HEAD if c.head else 0))
    options = dict(BASE_OPTIONS, **STEER[c.kernel])
    options.update(dict(c.opts), splitk=c.splitk)
    plane = c.B * H * W * coutp * 4
    scratch_planes = 0 if c.scratch is None else max(c.ksplit, _shape_ksplit(c, c0p + c1p)) + 1
    scratch_bytes = 0 if c.scratch is None else ((scratch_planes - 1) * plane - 1 if c.scratch == "short" else scratch_planes * plane)
    return dict(H=H, W=W, B=c.B, coutp=coutp, c0p=c0p, c1p=c1p, bn=bn, tiles=tiles, ntc=ntc, units=tiles * ntc, forms=forms, flags=flags, options=options, K=c.cin0 + c.cin1,
                H1=H // 2 if c.lowres else H, W1=W // 2 if c.lowres else W, Hp=(H + 1) // 2, Wp=(W + 1) // 2, scratch_planes=scratch_planes, scratch_bytes=scratch_bytes, plane=plane)


def _shape_ksplit(c: Case, cinp: int) -> int:
    """wino2d_ksplit_shape / wino4_ksplit_shape for a forced slice count (splitk >= 2): the K slices the shape allows, whatever the scratch holds."""
    if c.splitk < 2:
        return 1
    return max(1, min(c.splitk, cinp // 16 if c.kernel == K_WINO4 else cinp // 8))


def instantiation(c: Case, n_cu: int = CHIP_CUS) -> str:
    """The template instantiation the launchers dispatch the case to (their dispatch code restated)."""
    g = geometry(c, n_cu)
    k = c.kernel
    if k == K_REGSTAGED or k == K_WINO1D:
        return f"bn{g['bn']}"
    if k == K_DMA9:
        return ("persist" if g["options"]["persist"] else "tile") + f"_bn{g['bn']}"
    if k == K_C16:
        return ""
    if k == K_W16:
        chunks, nbs = (g["c0p"] + g["c1p"]) // 16, g["coutp"] // 16
        if c.head:
            return "1,1,head" if nbs == 1 else "2,2,head"
        if c.cin1:
            return "2,2,two" if nbs == 2 else f"{chunks},1,two"
        return f"{chunks},{nbs}"
    if k == K_WINO2D:
        if c.ksplit > 1:
            return "ks"
        ht, bwd = (g["coutp"] & 63) != 0 and (g["coutp"] & 63) <= 32, c.accumulate or c.mask
        return "ht_bwd" if ht and bwd else ("ht" if ht else ("bwd" if bwd else "plain"))
    if k == K_WINO4:
        return ("lowres_ks" if c.lowres else "ks") if c.ksplit > 1 else ("lowres" if c.lowres else "plain")
    units1 = c.B * ((g["H"] + 7) // 8) * ((g["W"] + 7) // 8) * (g["coutp"] // 16)
    nb = g["coutp"] // 16 if c.head else (2 if (g["coutp"] & 31) == 0 and units1 > n_cu else 1)
    return f"{'true' if c.lowres else 'false'},{nb}"


def expected_props(c: Case) -> int:
    """ConvRoute's property bits for the case's kernel (conv3x3_family_route / conv3x3_route restated)."""
    k = c.kernel
    if k == K_SMALLMAP:
        return P_LOWRES | (P_HEAD_SM if pad16(c.cout) <= 32 else 0)
    p = 0
    if k in (K_W16, K_WINO2D, K_WINO4) and not (c.pool or c.head or c.skip_dst):
        p |= P_MASK
    if k in (K_W16, K_WINO2D):
        p |= P_POOLS
    if k == K_WINO4:
        p |= P_LOWRES
    if k == K_WINO2D and c.ksplit <= 1:
        p |= P_HEAD_W2D
    if k == K_W16 and not c.cin1 and not c.pool and not c.mask and (pad16(c.cin0), pad16(c.cout)) in ((16, 16), (32, 32)):
        p |= P_HEAD_W16
    return p


# ---- operands

def _ints(gen, shape, lo, hi, step=1):
    return (torch.randint(lo // step, hi // step + 1, shape, generator=gen) * step).to(torch.float32)


def _nhwc(t, cp):
    """(B, H, W, c) -> (B, H, W, cp) with zero pad channels."""
    out = torch.zeros(*t.shape[:3], cp, dtype=t.dtype)
    out[..., : t.shape[3]] = t
    return out


def operands(c: Case, family: str, n_cu: int = CHIP_CUS, seed: int = 0) -> dict:
    """CPU float32 tensors: the sources as padded NHWC (pad channels zero), the canonical weight / bias / head weight / head bias, the old dst (every padded channel drawn)
    and the ReLU mask source in dst's layout."""
    g = geometry(c, n_cu)
    gen = torch.Generator().manual_seed(7000 + seed + sum(map(ord, c.name)))
    exact = family == "exact"
    draw = (lambda shape, lo=-4, hi=4, step=1: _ints(gen, shape, lo, hi, step)) if exact else (lambda shape, lo=0, hi=0, step=1: torch.rand(shape, generator=gen, dtype=torch.float32) - 0.5)
    o = {"src0": _nhwc(draw((g["B"], g["H"], g["W"], c.cin0)), g["c0p"]), "src1": None, "old": None, "mask": None, "head_w": None, "head_b": None}
    if c.cin1:
        s1 = draw((g["B"], g["H1"], g["W1"], c.cin1))
        o["src1"] = _nhwc(s1 * 16.0 if (exact and c.lowres) else s1, g["c1p"])
    halves = exact and c.kernel in (K_WINO1D, K_W16, K_WINO2D, K_SMALLMAP)
    o["weight"] = draw((c.cout, c.cin0 + c.cin1, 3, 3), -8, 8, 4) if halves else draw((c.cout, c.cin0 + c.cin1, 3, 3))
    o["bias"] = draw((c.cout,))
    if c.accumulate:
        o["old"] = draw((g["B"], g["H"], g["W"], g["coutp"]))
    if c.mask:
        o["mask"] = draw((g["B"], g["H"], g["W"], g["coutp"]))
    if c.head:
        o["head_w"] = draw((c.head, c.cout), -2, 2)
        o["head_b"] = draw((c.head,))
    return o


# ---- reference

def _nchw64(t, c):
    return t[..., :c].to(torch.float64).permute(0, 3, 1, 2)


def sources(c: Case, o: dict, dtype=torch.float64, magnitudes: bool = False):
    """The conv's input, NCHW of the true channel counts: src0 and (the up-sampled) src1 concatenated."""
    x = _nchw64(o["src0"], c.cin0).to(dtype)
    if c.cin1:
        s1 = _nchw64(o["src1"], c.cin1).to(dtype)
        if magnitudes:
            s1 = s1.abs()  # (the interpolation weights are positive)
        if c.lowres:
            s1 = F.interpolate(s1, scale_factor=2, mode="bilinear", align_corners=False)
        x = torch.cat([x.abs() if magnitudes else x, s1], 1)
    elif magnitudes:
        x = x.abs()
    return x


def _padc(t, cp):
    """(B, c, H, W) -> (B, cp, H, W), zero pad channels."""
    out = torch.zeros(t.shape[0], cp, *t.shape[2:], dtype=t.dtype)
    out[:, : t.shape[1]] = t
    return out


def epilogue(c: Case, g: dict, o: dict, conv, dtype=torch.float64) -> dict:
    """dst / pool / head from conv + bias (B, cout, H, W), every tensor in the layout the device stores: dst and pool NHWC of coutp channels, the head NCHW."""
    y = _padc(conv, g["coutp"])
    if c.relu:
        y = y.clamp(min=0.0)
    if c.accumulate:
        y = y + o["old"].to(dtype).permute(0, 3, 1, 2)
    if c.mask:
        y = torch.where(o["mask"].permute(0, 3, 1, 2) > 0, y, torch.zeros_like(y))
    out = {"dst": y.permute(0, 2, 3, 1).contiguous(), "pool": None, "head_pre": None, "head": None}
    if c.pool:
        assert c.relu == 1, "pool cases run with relu = 1: beyond the image the kernels' pool counts zeros"
        out["pool"] = F.max_pool2d(y, 2, 2, ceil_mode=True).permute(0, 2, 3, 1).contiguous()
    if c.head:
        hw = torch.zeros(c.head, g["coutp"], dtype=dtype)
        hw[:, : c.cout] = o["head_w"].to(dtype)
        pre = torch.einsum("oc,bchw->bohw", hw, y) + o["head_b"].to(dtype).view(1, -1, 1, 1)
        out["head_pre"] = pre
        out["head"] = torch.sigmoid(pre) if c.sigmoid else pre
    return out


def reference(c: Case, o: dict, n_cu: int = CHIP_CUS) -> dict:
    """-> dst, pool, head_pre, head (float64, device layouts), S and S_head (the magnitude sums of dst and of the head's pre-activation)."""
    g = geometry(c, n_cu)
    w, b = o["weight"].to(torch.float64), o["bias"].to(torch.float64)
    conv = F.conv2d(sources(c, o), w, padding=1) + b.view(1, -1, 1, 1)
    out = epilogue(c, g, o, conv)
    S = _padc(F.conv2d(sources(c, o, magnitudes=True), w.abs(), padding=1) + b.abs().view(1, -1, 1, 1), g["coutp"])
    if c.accumulate:
        S = S + o["old"].to(torch.float64).abs().permute(0, 3, 1, 2)
    out["S"] = S.permute(0, 2, 3, 1).contiguous()
    out["conv"] = conv
    if c.head:
        out["S_head"] = torch.einsum("oc,bchw->bohw", o["head_w"].to(torch.float64).abs(), out["dst"].permute(0, 3, 1, 2)[:, : c.cout].abs()) + o["head_b"].to(torch.float64).abs().view(1, -1, 1, 1)
    return out


# ---- the textbook Winograd algorithms, in any dtype (float32: the reference's own evaluation; float64 on magnitudes: the rigorous bound)

_MATS = {
    2: ([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]], [[1, 0, 0], [0.5, 0.5, 0.5], [0.5, -0.5, 0.5], [0, 0, 1]], [[1, 1, 1, 0], [0, 1, -1, -1]]),
    4: ([[4, 0, -5, 0, 1, 0], [0, -4, -4, 1, 1, 0], [0, 4, -4, -1, 1, 0], [0, -2, -1, 2, 1, 0], [0, 2, -1, -2, 1, 0], [0, 4, 0, -5, 0, 1]],
        [[1 / 4, 0, 0], [-1 / 6, -1 / 6, -1 / 6], [-1 / 6, 1 / 6, -1 / 6], [1 / 24, 1 / 12, 1 / 6], [1 / 24, -1 / 12, 1 / 6], [0, 0, 1]],
        [[1, 1, 1, 1, 1, 0], [0, 1, -1, 2, -2, 0], [0, 1, 1, 4, 4, 0], [0, 1, -1, 8, -8, 1]]),
}


def winograd(x, w, m: int, two_d: bool, magnitudes: bool = False):
    """F(m x m, 3x3) (two_d) or F(m, 3) along x of NCHW `x` with OIHW `w`, "same" padding, in x's dtype.  magnitudes: the matrices' absolute values on |x|, |w|."""
    dt = x.dtype
    BT, G, AT = (torch.tensor(t, dtype=torch.float64) for t in _MATS[m])
    if magnitudes:
        BT, G, AT, x, w = BT.abs(), G.abs(), AT.abs(), x.abs(), w.abs()
    BT, G, AT = BT.to(dt), G.to(dt), AT.to(dt)  # (G of F(4,3): 1/6, 1/12, 1/24 rounded to dt, as the device's fp32 constants are)
    B, C, H, W = x.shape
    a = m + 2
    Wt = (W + m - 1) // m
    Ht = (H + m - 1) // m if two_d else H
    xp = torch.zeros(B, C, (Ht * m if two_d else H) + 2, Wt * m + 2, dtype=dt)
    xp[:, :, 1 : H + 1, 1 : W + 1] = x
    if two_d:
        d = xp.unfold(2, a, m).unfold(3, a, m)  # (B, C, Ht, Wt, a, a)
        V = torch.einsum("ij,bcyxjk,lk->bcyxil", BT, d, BT)
        Uw = torch.einsum("ij,ocjk,lk->ocil", G, w, G)
        M = torch.einsum("ocil,bcyxil->boyxil", Uw, V)
        Y = torch.einsum("pi,boyxil,ql->boypxq", AT, M, AT).reshape(B, w.shape[0], Ht * m, Wt * m)
    else:
        d = xp.unfold(3, a, m)  # (B, C, H + 2, Wt, a)
        V = torch.einsum("ij,bcyxj->bcyxi", BT, d)
        Uw = torch.einsum("ij,ockj->ocki", G, w)  # (O, C, ky, a)
        M = sum(torch.einsum("oci,bcyxi->boyxi", Uw[:, :, ky], V[:, :, ky : ky + H]) for ky in range(3))
        Y = torch.einsum("pi,boyxi->boyxp", AT, M).reshape(B, w.shape[0], H, Wt * m)
    return Y[:, :, :H, :W].contiguous()


def fp32_evaluation(c: Case, o: dict, n_cu: int = CHIP_CUS) -> dict:
    """The case's own algorithm in float32 on the CPU (the fold, the transforms, the bias, the epilogue) -> the tensors of `reference`, float32."""
    g = geometry(c, n_cu)
    m, two_d = WINO_M[c.kernel]
    conv = winograd(sources(c, o, dtype=torch.float32), o["weight"], m, two_d) + o["bias"].view(1, -1, 1, 1)
    return epilogue(c, g, o, conv, dtype=torch.float32)


def rigorous_bound(c: Case, o: dict, n_cu: int = CHIP_CUS):
    """Per element of dst (NHWC, coutp): gamma_n x the magnitude sum through the absolute-value transforms (+ |bias|, + |old dst|)."""
    g = geometry(c, n_cu)
    m, two_d = WINO_M[c.kernel]
    mag = winograd(sources(c, o, magnitudes=True), o["weight"].to(torch.float64), m, two_d, magnitudes=True) + o["bias"].to(torch.float64).abs().view(1, -1, 1, 1)
    mag = _padc(mag, g["coutp"])
    if c.accumulate:
        mag = mag + o["old"].to(torch.float64).abs().permute(0, 3, 1, 2)
    return gamma(g["K"] + WINO_ROUNDINGS) * mag.permute(0, 2, 3, 1).contiguous(), mag.permute(0, 2, 3, 1).contiguous()


def e32_of(c: Case, o: dict, ref: dict, n_cu: int = CHIP_CUS) -> float:
    return float((fp32_evaluation(c, o, n_cu)["dst"].to(torch.float64) - ref["dst"]).abs().max())


def case_e32(c: Case, o: dict, ref: dict, n_cu: int = CHIP_CUS) -> float:
    """e32 of a float case: the recorded value where the case's map is the recorded one, else recomputed (always from the reference alone)."""
    g, g0 = geometry(c, n_cu), geometry(c, CHIP_CUS)
    return MEASURED[c.name] if (g0["H"], g0["W"]) == (g["H"], g["W"]) and c.name in MEASURED else e32_of(c, o, ref, n_cu)


def dst_bar(c: Case, o: dict, ref: dict, n_cu: int = CHIP_CUS, e32: Optional[float] = None):
    """The float family's bar per element of dst (NHWC, coutp)."""
    if c.direct:
        return gamma(9 * geometry(c, n_cu)["K"] + 3) * ref["S"]
    rig, _ = rigorous_bound(c, o, n_cu)
    return torch.minimum(torch.full_like(rig, 4.0 * (case_e32(c, o, ref, n_cu) if e32 is None else e32)), rig)


def head_bar(c: Case, o: dict, ref: dict, bar):
    """The bar of the fused head's pre-activation (NCHW): the conv's bar through sum |head_w| (ReLU and the mask do not enlarge an error), then the head's own sum."""
    g = geometry(c)
    through = torch.einsum("oc,bhwc->bohw", o["head_w"].to(torch.float64).abs(), bar[..., : c.cout])
    return through + gamma(g["coutp"] + 2) * (ref["S_head"] + through)


# ---- the case table: per kernel the smallest shapes on its own tile edges

def _rows_past(kernel, rounds, ntc=1, grid_per_cu=1, cols=3, multiple=1, B=3):
    """H(n_cu) of a B-image map `cols` tiles wide whose units (tiles x ntc) just exceed `rounds` rounds of the persistent grid; the last tile row is partial."""
    th = TILE[kernel][0]

    def H(n_cu):
        ty = rounds * n_cu * grid_per_cu // (B * cols * ntc) + 1
        return ty * th - (4 if multiple == 4 else 3)
    return H


def _sm_cols(n_cu):  # 8 x 8-pixel units of three images x two N blocks just past the CU count: the small-map kernel takes two N blocks per workgroup
    return 8 * (n_cu // 6 + 1) - 2


def _table():
    t = []

    def add(name, kernel, **kw):
        t.append(Case(name, kernel, **kw))

    def edges(kernel, multiple=1):
        th, tw = TILE[kernel]
        if multiple == 4:
            return [(th - 4, tw - 4), (th, tw), (th + 4, tw + 4)]
        return [(th - 1, tw - 1), (th, tw), (th + 1, tw + 1)]

    tiny = [(1, 1), (2, 3), (3, 2), (1, 5)]
    # ---- the three kernels without transformed weights and F(2,3) along x: N tiles of 32 and of 64, the same edges each
    for kernel, tag in ((K_REGSTAGED, "reg"), (K_DMA9, "dma9"), (K_WINO1D, "wino1d")):
        ch = [(40, 18, 27), (16, 16, 0), (32, 48, 0), (64, 32, 16), (96, 16, 16), (128, 16, 0), (48, 16, 0)]  # (cout, cin0, cin1): coutp 48, 16, 32 | 64, 96, 128 | 48
        for i, (H, W) in enumerate(edges(kernel)):
            cout, cin0, cin1 = ch[i]
            add(f"{tag}_bn32_{H}x{W}", kernel, cout=cout, cin0=cin0, cin1=cin1, H=H, W=W, relu=i & 1, tags=("pair",))
            cout, cin0, cin1 = ch[3 + i]
            add(f"{tag}_bn64_{H}x{W}", kernel, cout=cout, cin0=cin0, cin1=cin1, H=H, W=W, relu=1 - (i & 1), tags=("pair",))
        for i, (H, W) in enumerate(tiny):
            add(f"{tag}_tiny_{H}x{W}", kernel, cout=(40, 64)[i & 1], cin0=18, cin1=27 if i < 2 else 0, H=H, W=W)
        th, tw = TILE[kernel]
        add(f"{tag}_accumulate_bn32", kernel, cout=40, cin0=24, H=th + 1, W=tw + 1, accumulate=True)
        add(f"{tag}_accumulate_bn64", kernel, cout=96, cin0=24, H=th + 1, W=tw + 1, accumulate=True, relu=0)
        add(f"{tag}_pool_odd_bn32", kernel, cout=40, cin0=24, H=th + 1, W=tw + 3, pool=True)
        add(f"{tag}_pool_odd_bn64", kernel, cout=96, cin0=18, cin1=27, H=2 * th - 1, W=tw - 1, pool=True)
        add(f"{tag}_k3chunks", kernel, cout=48, cin0=48, H=th - 1, W=tw + 1)
    add("wino1d_pool_skip_dst", K_WINO1D, cout=40, cin0=24, H=17, W=35, pool=True, skip_dst=True)
    add("wino1d_pool_skip_dst_bn64", K_WINO1D, cout=64, cin0=24, H=15, W=33, pool=True, skip_dst=True)
    for bn_cout, tag in ((40, "bn32"), (128, "bn64")):
        for H, W in ((15, 31), (17, 33)):
            add(f"dma9_tile_{tag}_{H}x{W}", K_DMA9, cout=bn_cout, cin0=18, cin1=27, H=H, W=W, opts=(("persist", 0),), tags=("pair",))
    add("dma9_tile_pool", K_DMA9, cout=96, cin0=24, H=17, W=33, opts=(("persist", 0),), pool=True)
    add("dma9_tile_accumulate", K_DMA9, cout=40, cin0=24, H=17, W=33, opts=(("persist", 0),), accumulate=True)
    # past the first tile of the persistent grid: units just above one and just above two rounds of the chip, two N tiles (a (pixel tile, N tile) pair done twice or never)
    for rounds in (1, 2):
        add(f"dma9_rounds{rounds}_bn64", K_DMA9, cout=128, cin0=16, H=_rows_past(K_DMA9, rounds, 2), W=91, tags=("rounds",))
        add(f"dma9_rounds{rounds}_bn32", K_DMA9, cout=40, cin0=16, H=_rows_past(K_DMA9, rounds, 2), W=91, tags=("rounds",))
        add(f"wino1d_rounds{rounds}_bn64", K_WINO1D, cout=128, cin0=16, H=_rows_past(K_WINO1D, rounds, 2), W=91, tags=("rounds",))
        add(f"wino1d_rounds{rounds}_bn32", K_WINO1D, cout=40, cin0=16, H=_rows_past(K_WINO1D, rounds, 2), W=91, tags=("rounds",))
        add(f"c16_rounds{rounds}", K_C16, cout=16, cin0=16, H=_rows_past(K_C16, rounds, 1, 4), W=91, tags=("rounds",))
        add(f"w16_rounds{rounds}", K_W16, cout=32, cin0=32, H=_rows_past(K_W16, rounds), W=45, tags=("rounds",))
        add(f"wino2d_rounds{rounds}", K_WINO2D, cout=128, cin0=32, H=_rows_past(K_WINO2D, rounds, 2), W=45, tags=("rounds",))
        add(f"wino4_rounds{rounds}", K_WINO4, cout=128, cin0=64, H=_rows_past(K_WINO4, rounds, 2, multiple=4), W=92, tags=("rounds",))
    add("dma9_tile_many_units", K_DMA9, cout=128, cin0=16, H=_rows_past(K_DMA9, 1, 2), W=91, opts=(("persist", 0),), tags=("rounds",))
    # ---- conv3x3_c16
    for i, (H, W) in enumerate(edges(K_C16) + tiny):
        add(f"c16_{H}x{W}", K_C16, cout=(16, 11)[i & 1], cin0=(16, 5)[(i >> 1) & 1], H=H, W=W, relu=i & 1, tags=("pair",))
    add("c16_accumulate", K_C16, cout=16, cin0=16, H=9, W=33, accumulate=True)
    # ---- the wave-private F(2x2,3x3) kernel: every instantiation, every c0p : c1p split of w16_shape_ok
    w16_shapes = {"1,1": (16, 16, 0), "2,1": (11, 32, 0), "1,2": (32, 16, 0), "2,2": (27, 18, 0), "2,1,two": (16, 16, 16), "3,1,two": (16, 16, 32), "4,1,two": (16, 16, 48),
                  "2,2,two": (32, 16, 16)}
    for i, (inst, (cout, cin0, cin1)) in enumerate(w16_shapes.items()):
        for j, (H, W) in enumerate(edges(K_W16)):
            add(f"w16_{inst.replace(',', '_')}_{H}x{W}", K_W16, cout=cout, cin0=cin0, cin1=cin1, H=H, W=W, relu=(i + j) & 1, pool=(j == 2 and (i + j) & 1 == 1), tags=("pair",))
    for cin0, cin1 in ((32, 16), (32, 32), (48, 16), (27, 18)):  # the other splits: chunks of source 0 even and odd; true counts no multiple of 16
        add(f"w16_split_{cin0}_{cin1}", K_W16, cout=13, cin0=cin0, cin1=cin1, H=33, W=17)
    for i, (H, W) in enumerate(tiny):
        add(f"w16_tiny_{H}x{W}", K_W16, cout=(16, 32)[i & 1], cin0=(16, 32)[i >> 1], cin1=0, H=H, W=W)
    add("w16_mask", K_W16, cout=32, cin0=16, H=33, W=17, mask=True)
    add("w16_mask_two", K_W16, cout=16, cin0=16, cin1=32, H=31, W=17, mask=True, relu=0)
    add("w16_pool_skip_dst", K_W16, cout=32, cin0=32, H=33, W=15, pool=True, skip_dst=True)
    add("w16_pool_odd_two", K_W16, cout=16, cin0=16, cin1=16, H=35, W=19, pool=True)
    for hc in (1, 16):
        for sig in (False, True):
            add(f"w16_head{hc}_16_sig{int(sig)}", K_W16, cout=16, cin0=16, H=33, W=17 + int(sig), head=hc, sigmoid=sig, tags=("pair",))
            add(f"w16_head{hc}_32_sig{int(sig)}", K_W16, cout=27, cin0=18, H=31, W=16 - int(sig), head=hc, sigmoid=sig, skip_dst=sig, tags=("pair",))
    # ---- the wave-split F(2x2,3x3) kernel
    w2_ch = [(64, 32, 0), (96, 18, 27), (128, 48, 0)]  # coutp 64, 96 (half-empty last tile), 128
    for i, (H, W) in enumerate(edges(K_WINO2D)):
        cout, cin0, cin1 = w2_ch[i]
        add(f"wino2d_{H}x{W}_cout{cout}", K_WINO2D, cout=cout, cin0=cin0, cin1=cin1, H=H, W=W, relu=i & 1, tags=("pair",))
    add("wino2d_n64_cout32", K_WINO2D, cout=32, cin0=64, bn=64, H=17, W=15, tags=("pair",))          # the half-empty-tile packing of a 32-channel layer
    add("wino2d_n64_cout27_two", K_WINO2D, cout=27, cin0=40, cin1=24, bn=64, H=15, W=17, relu=0, tags=("pair",))
    add("wino2d_ht_cout96_pool", K_WINO2D, cout=96, cin0=32, H=17, W=19, pool=True, tags=("pair",))
    for i, (H, W) in enumerate(tiny):
        add(f"wino2d_tiny_{H}x{W}", K_WINO2D, cout=(64, 96)[i & 1], cin0=32, cin1=16 if i < 2 else 0, H=H, W=W)
    add("wino2d_accumulate", K_WINO2D, cout=64, cin0=32, H=17, W=15, accumulate=True, tags=("pair",))
    add("wino2d_mask", K_WINO2D, cout=128, cin0=32, H=15, W=17, mask=True, relu=0, tags=("pair",))
    add("wino2d_accumulate_mask", K_WINO2D, cout=64, cin0=18, cin1=27, H=17, W=17, accumulate=True, mask=True)
    add("wino2d_ht_accumulate", K_WINO2D, cout=96, cin0=32, H=17, W=15, accumulate=True, tags=("pair",))
    add("wino2d_ht_mask_n64", K_WINO2D, cout=32, cin0=64, bn=64, H=15, W=17, mask=True, tags=("pair",))
    add("wino2d_ht_accumulate_mask", K_WINO2D, cout=96, cin0=32, cin1=16, H=17, W=17, accumulate=True, mask=True, relu=0)
    add("wino2d_pool_odd", K_WINO2D, cout=128, cin0=32, H=17, W=19, pool=True)
    add("wino2d_pool_skip_dst", K_WINO2D, cout=64, cin0=48, H=15, W=17, pool=True, skip_dst=True)
    for hc in (1, 17, 32):
        for sig in (False, True):
            add(f"wino2d_head{hc}_sig{int(sig)}", K_WINO2D, cout=(64, 50)[int(sig)], cin0=32, cin1=16 * int(sig), H=17, W=16 + int(sig), head=hc, sigmoid=sig, skip_dst=(hc == 17))
    for ks in (2, 3):
        for fin in (0, 1):
            add(f"wino2d_splitk{ks}_finish{fin}", K_WINO2D, cout=(64, 128)[fin], cin0=48, H=17, W=15, splitk=ks, scratch="fits", splitk_finish=fin, ksplit=ks, relu=fin, tags=("pair",))
    add("wino2d_splitk_clamped", K_WINO2D, cout=64, cin0=32, H=17, W=17, splitk=7, scratch="fits", ksplit=4)            # 32 input channels: four slices of one 8-channel half
    add("wino2d_splitk_clamped_finish", K_WINO2D, cout=64, cin0=32, H=15, W=17, splitk=7, scratch="fits", ksplit=4, splitk_finish=1)
    add("wino2d_splitk_pool", K_WINO2D, cout=64, cin0=48, H=17, W=19, splitk=2, scratch="fits", ksplit=2, pool=True)
    add("wino2d_splitk_pool_finish", K_WINO2D, cout=128, cin0=32, H=17, W=19, splitk=3, scratch="fits", ksplit=3, pool=True, splitk_finish=1)
    add("wino2d_splitk_pool_skip_dst", K_WINO2D, cout=64, cin0=48, H=15, W=17, splitk=2, scratch="fits", ksplit=2, pool=True, skip_dst=True)
    add("wino2d_splitk_pool_skip_dst_finish", K_WINO2D, cout=64, cin0=48, H=15, W=17, splitk=2, scratch="fits", ksplit=2, pool=True, skip_dst=True, splitk_finish=1)
    add("wino2d_splitk_half_empty_refused", K_WINO2D, cout=96, cin0=48, H=17, W=15, splitk=2, scratch="fits", ksplit=1)  # the half-empty-tile instantiation has no split form
    add("wino2d_splitk_scratch_short", K_WINO2D, cout=64, cin0=48, H=17, W=15, splitk=2, scratch="short", ksplit=1)      # one byte too small: one stage (launch_ksplit)
    add("wino2d_splitk_accumulate_refused", K_WINO2D, cout=64, cin0=48, H=17, W=15, splitk=2, scratch="fits", ksplit=1, accumulate=True)
    # ---- F(4x4,3x3): H, W multiples of 4, K from 64 on
    w4_ch = [(64, 64, 0), (96, 40, 24), (128, 80, 0)]
    for i, (H, W) in enumerate(edges(K_WINO4, 4)):
        cout, cin0, cin1 = w4_ch[i]
        add(f"wino4_{H}x{W}_cout{cout}", K_WINO4, cout=cout, cin0=cin0, cin1=cin1, H=H, W=W, relu=i & 1, tags=("pair",))
    add("wino4_4x4", K_WINO4, cout=72, cin0=64, H=4, W=4, tags=("pair",))
    add("wino4_n64_cout32", K_WINO4, cout=32, cin0=64, bn=64, H=20, W=36)
    add("wino4_mask", K_WINO4, cout=64, cin0=64, H=20, W=28, mask=True, relu=0)
    add("wino4_pool", K_WINO4, cout=96, cin0=64, H=20, W=36, pool=True)
    add("wino4_pool_skip_dst", K_WINO4, cout=64, cin0=18, cin1=50, H=12, W=36, pool=True, skip_dst=True)
    for H, W in ((4, 4), (12, 28), (20, 36)):  # the clamped low-resolution indices against the zero padding of the up-sampled tensor, at all four borders
        add(f"wino4_lowres_{H}x{W}", K_WINO4, cout=64, cin0=32, cin1=32, H=H, W=W, lowres=True, tags=("pair",))
    add("wino4_lowres_odd_channels", K_WINO4, cout=72, cin0=18, cin1=50, H=20, W=36, lowres=True, relu=0, tags=("pair",))
    add("wino4_lowres_pool", K_WINO4, cout=64, cin0=16, cin1=64, H=20, W=28, lowres=True, pool=True)
    for ks in (2, 3):
        add(f"wino4_splitk{ks}", K_WINO4, cout=(64, 128)[ks - 2], cin0=128, H=20, W=36, splitk=ks, scratch="fits", ksplit=ks, relu=ks & 1, tags=("pair",))
        add(f"wino4_lowres_splitk{ks}", K_WINO4, cout=64, cin0=64, cin1=64, H=12, W=36, lowres=True, splitk=ks, scratch="fits", ksplit=ks, tags=("pair",))
    add("wino4_splitk_clamped", K_WINO4, cout=64, cin0=128, H=20, W=28, splitk=11, scratch="fits", ksplit=8)   # 128 input channels: eight slices of four quarters
    add("wino4_splitk_pool", K_WINO4, cout=64, cin0=128, H=20, W=36, splitk=2, scratch="fits", ksplit=2, pool=True)
    add("wino4_splitk_pool_skip_dst", K_WINO4, cout=64, cin0=128, H=12, W=28, splitk=2, scratch="fits", ksplit=2, pool=True, skip_dst=True)
    add("wino4_splitk_scratch_short", K_WINO4, cout=64, cin0=128, H=20, W=36, splitk=2, scratch="short", ksplit=1)
    add("wino4_splitk_short_k", K_WINO4, cout=64, cin0=64, H=20, W=36, splitk=2, scratch="fits", ksplit=1)    # fewer than 128 input channels: no split
    # ---- the small-map kernel
    sm_ch = [(16, 16, 0), (40, 18, 27), (64, 48, 0)]
    for i, (H, W) in enumerate(edges(K_SMALLMAP)):
        cout, cin0, cin1 = sm_ch[i]
        add(f"sm_{H}x{W}_cout{cout}", K_SMALLMAP, cout=cout, cin0=cin0, cin1=cin1, H=H, W=W, relu=i & 1, tags=("pair",))
    for i, (H, W) in enumerate(tiny):
        add(f"sm_tiny_{H}x{W}", K_SMALLMAP, cout=(96, 128)[i & 1], cin0=32, cin1=16 if i < 2 else 0, H=H, W=W)
    add("sm_pool_odd", K_SMALLMAP, cout=40, cin0=24, H=9, W=11, pool=True)
    add("sm_pool_skip_dst", K_SMALLMAP, cout=32, cin0=48, H=7, W=9, pool=True, skip_dst=True)
    add("sm_two_blocks", K_SMALLMAP, cout=32, cin0=18, cin1=27, H=9, W=_sm_cols, tags=("pair",))
    add("sm_two_blocks_pool", K_SMALLMAP, cout=64, cin0=16, H=7, W=_sm_cols, pool=True, tags=("pair",))
    for H, W in ((2, 2), (4, 4), (8, 8), (10, 6)):
        add(f"sm_lowres_{H}x{W}", K_SMALLMAP, cout=40, cin0=18, cin1=27, H=H, W=W, lowres=True, tags=("pair",))
    add("sm_lowres_pool", K_SMALLMAP, cout=16, cin0=16, cin1=48, H=10, W=14, lowres=True, pool=True, tags=("pair",))
    add("sm_lowres_two_blocks", K_SMALLMAP, cout=32, cin0=16, cin1=16, H=10, W=_sm_cols, lowres=True, tags=("pair",))
    add("sm_lowres_two_blocks_relu0", K_SMALLMAP, cout=64, cin0=16, cin1=32, H=6, W=_sm_cols, lowres=True, relu=0, tags=("pair",))
    for hc in (1, 17):
        for sig in (False, True):
            add(f"sm_head{hc}_sig{int(sig)}", K_SMALLMAP, cout=(16, 27)[int(sig)], cin0=24, cin1=16 * int(sig), H=9, W=10 + int(sig), head=hc, sigmoid=sig, skip_dst=sig)
    add("sm_head_lowres", K_SMALLMAP, cout=32, cin0=16, cin1=16, H=10, W=6, lowres=True, head=5)
    return t


CASES = _table()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES), "case names must be unique"
CROSS_CHECK = ("wino2d_15x15_cout64", (K_DMA9, K_WINO1D, K_REGSTAGED))  # the same float operands through other kernels, each held to the reference on its own


def missing_coverage(cases, n_cu: int = CHIP_CUS) -> list:
    """The (kernel, instantiation) pairs of PAIRS for which `cases` holds fewer than two "pair" cases (two, so that ONE case of a pair cannot leave unnoticed), and the
    epilogue forms ConvRoute allows a kernel and no case gives it."""
    have = {}
    for c in cases:
        if "pair" in c.tags:
            have.setdefault((c.kernel, instantiation(c, n_cu)), []).append(c.name)
    missing = [("pair", k, i) for k, i in PAIRS if len(have.get((k, i), [])) < 2]
    for k in range(8):
        mine = [c for c in cases if c.kernel == k]
        want = {"relu0": lambda c: c.relu == 0, "relu1": lambda c: c.relu == 1}
        if k not in (K_W16, K_WINO4, K_SMALLMAP):
            want["accumulate"] = lambda c: c.accumulate
        if k in (K_W16, K_WINO2D, K_WINO4):
            want["mask"] = lambda c: c.mask
        if k != K_C16:
            want["pool"] = lambda c: c.pool and not c.skip_dst
        if k in (K_WINO1D, K_W16, K_WINO2D, K_WINO4, K_SMALLMAP):
            want["pool_skip_dst"] = lambda c: c.pool and c.skip_dst
        if k in (K_W16, K_WINO2D, K_SMALLMAP):
            want["head"] = lambda c: c.head and not c.sigmoid
            want["head_sigmoid"] = lambda c: c.head and c.sigmoid
        if k in (K_WINO4, K_SMALLMAP):
            want["lowres"] = lambda c: c.lowres
        if k in (K_WINO2D, K_WINO4):
            want["splitk"] = lambda c: c.ksplit > 1
        if k in PERSISTENT:
            want["rounds"] = lambda c: "rounds" in c.tags
        missing += [("epilogue", k, name) for name, f in want.items() if not any(f(c) for c in mine)]
    return missing


# e32 per float case of a Winograd kernel at the geometry of a 256-CU chip: max |fp32 - float64| of the reference's own float32 evaluation (fp32_evaluation), written by
# test_conv3x3_cpu.py under CONV3X3_RECORD=1.  Nothing here comes from a device run.
# MEASURED-BEGIN
MEASURED = {
    "wino1d_bn32_15x31": 1.5041e-06,
    "wino1d_bn64_15x31": 1.5971e-06,
    "wino1d_bn32_16x32": 5.9900e-07,
    "wino1d_bn64_16x32": 1.4128e-06,
    "wino1d_bn32_17x33": 1.6452e-06,
    "wino1d_bn64_17x33": 7.5499e-07,
    "wino1d_tiny_1x1": 2.6857e-07,
    "wino1d_tiny_2x3": 7.5916e-07,
    "wino1d_tiny_3x2": 3.7822e-07,
    "wino1d_tiny_1x5": 2.7555e-07,
    "wino1d_accumulate_bn32": 9.0227e-07,
    "wino1d_accumulate_bn64": 9.7149e-07,
    "wino1d_pool_odd_bn32": 8.9456e-07,
    "wino1d_pool_odd_bn64": 1.7779e-06,
    "wino1d_k3chunks": 1.6956e-06,
    "wino1d_pool_skip_dst": 8.5035e-07,
    "wino1d_pool_skip_dst_bn64": 9.3776e-07,
    "wino1d_rounds1_bn64": 8.9024e-07,
    "wino1d_rounds1_bn32": 7.5386e-07,
    "w16_rounds1": 1.9194e-06,
    "wino2d_rounds1": 1.9931e-06,
    "wino4_rounds1": 6.7307e-05,
    "wino1d_rounds2_bn64": 8.7923e-07,
    "wino1d_rounds2_bn32": 8.7449e-07,
    "w16_rounds2": 2.0902e-06,
    "wino2d_rounds2": 2.0294e-06,
    "wino4_rounds2": 1.0170e-04,
    "w16_1_1_31x15": 8.0621e-07,
    "w16_1_1_32x16": 7.2072e-07,
    "w16_1_1_33x17": 8.0088e-07,
    "w16_2_1_31x15": 1.1916e-06,
    "w16_2_1_32x16": 1.1088e-06,
    "w16_2_1_33x17": 1.2916e-06,
    "w16_1_2_31x15": 8.1255e-07,
    "w16_1_2_32x16": 6.8238e-07,
    "w16_1_2_33x17": 9.4727e-07,
    "w16_2_2_31x15": 9.5161e-07,
    "w16_2_2_32x16": 7.8972e-07,
    "w16_2_2_33x17": 1.0081e-06,
    "w16_2_1_two_31x15": 1.3563e-06,
    "w16_2_1_two_32x16": 1.4424e-06,
    "w16_2_1_two_33x17": 1.2419e-06,
    "w16_3_1_two_31x15": 1.7994e-06,
    "w16_3_1_two_32x16": 1.8887e-06,
    "w16_3_1_two_33x17": 1.8337e-06,
    "w16_4_1_two_31x15": 3.0232e-06,
    "w16_4_1_two_32x16": 3.1962e-06,
    "w16_4_1_two_33x17": 2.6616e-06,
    "w16_2_2_two_31x15": 1.4053e-06,
    "w16_2_2_two_32x16": 1.4240e-06,
    "w16_2_2_two_33x17": 1.3314e-06,
    "w16_split_32_16": 2.1894e-06,
    "w16_split_32_32": 2.6304e-06,
    "w16_split_48_16": 2.6658e-06,
    "w16_split_27_18": 1.9535e-06,
    "w16_tiny_1x1": 1.1897e-07,
    "w16_tiny_2x3": 4.1054e-07,
    "w16_tiny_3x2": 5.2703e-07,
    "w16_tiny_1x5": 4.9567e-07,
    "w16_mask": 7.5177e-07,
    "w16_mask_two": 1.9593e-06,
    "w16_pool_skip_dst": 1.2649e-06,
    "w16_pool_odd_two": 1.5235e-06,
    "w16_head1_16_sig0": 7.0575e-07,
    "w16_head1_32_sig0": 1.0510e-06,
    "w16_head1_16_sig1": 6.9131e-07,
    "w16_head1_32_sig1": 8.3290e-07,
    "w16_head16_16_sig0": 6.0124e-07,
    "w16_head16_32_sig0": 9.1734e-07,
    "w16_head16_16_sig1": 8.3987e-07,
    "w16_head16_32_sig1": 9.0678e-07,
    "wino2d_15x15_cout64": 1.4518e-06,
    "wino2d_16x16_cout96": 2.5666e-06,
    "wino2d_17x17_cout128": 2.3409e-06,
    "wino2d_n64_cout32": 3.0414e-06,
    "wino2d_n64_cout27_two": 2.7988e-06,
    "wino2d_ht_cout96_pool": 1.6440e-06,
    "wino2d_tiny_1x1": 3.7627e-07,
    "wino2d_tiny_2x3": 9.7796e-07,
    "wino2d_tiny_3x2": 7.0588e-07,
    "wino2d_tiny_1x5": 5.2695e-07,
    "wino2d_accumulate": 1.2164e-06,
    "wino2d_mask": 1.3589e-06,
    "wino2d_accumulate_mask": 1.8453e-06,
    "wino2d_ht_accumulate": 1.4762e-06,
    "wino2d_ht_mask_n64": 2.0288e-06,
    "wino2d_ht_accumulate_mask": 2.2865e-06,
    "wino2d_pool_odd": 1.3690e-06,
    "wino2d_pool_skip_dst": 2.0638e-06,
    "wino2d_head1_sig0": 1.5300e-06,
    "wino2d_head1_sig1": 1.7435e-06,
    "wino2d_head17_sig0": 1.4724e-06,
    "wino2d_head17_sig1": 2.1602e-06,
    "wino2d_head32_sig0": 1.3323e-06,
    "wino2d_head32_sig1": 1.8076e-06,
    "wino2d_splitk2_finish0": 2.3056e-06,
    "wino2d_splitk2_finish1": 2.0810e-06,
    "wino2d_splitk3_finish0": 1.9775e-06,
    "wino2d_splitk3_finish1": 2.0592e-06,
    "wino2d_splitk_clamped": 1.3016e-06,
    "wino2d_splitk_clamped_finish": 1.3479e-06,
    "wino2d_splitk_pool": 2.0588e-06,
    "wino2d_splitk_pool_finish": 1.3747e-06,
    "wino2d_splitk_pool_skip_dst": 1.9860e-06,
    "wino2d_splitk_pool_skip_dst_finish": 1.8114e-06,
    "wino2d_splitk_half_empty_refused": 2.0461e-06,
    "wino2d_splitk_scratch_short": 2.5502e-06,
    "wino2d_splitk_accumulate_refused": 1.8175e-06,
    "wino4_12x28_cout64": 5.8780e-05,
    "wino4_16x32_cout96": 6.2535e-05,
    "wino4_20x36_cout128": 7.6429e-05,
    "wino4_4x4": 3.0189e-05,
    "wino4_n64_cout32": 4.5952e-05,
    "wino4_mask": 4.9690e-05,
    "wino4_pool": 5.3803e-05,
    "wino4_pool_skip_dst": 6.8563e-05,
    "wino4_lowres_4x4": 2.6317e-05,
    "wino4_lowres_12x28": 3.6285e-05,
    "wino4_lowres_20x36": 5.9103e-05,
    "wino4_lowres_odd_channels": 3.9727e-05,
    "wino4_lowres_pool": 4.1109e-05,
    "wino4_splitk2": 1.0647e-04,
    "wino4_lowres_splitk2": 7.4547e-05,
    "wino4_splitk3": 1.0909e-04,
    "wino4_lowres_splitk3": 8.3280e-05,
    "wino4_splitk_clamped": 8.9891e-05,
    "wino4_splitk_pool": 9.1109e-05,
    "wino4_splitk_pool_skip_dst": 8.9186e-05,
    "wino4_splitk_scratch_short": 1.1805e-04,
    "wino4_splitk_short_k": 4.7146e-05,
    "sm_7x7_cout16": 5.6961e-07,
    "sm_8x8_cout40": 1.4553e-06,
    "sm_9x9_cout64": 2.0619e-06,
    "sm_tiny_1x1": 2.6198e-07,
    "sm_tiny_2x3": 1.0945e-06,
    "sm_tiny_3x2": 9.4414e-07,
    "sm_tiny_1x5": 5.9169e-07,
    "sm_pool_odd": 8.3070e-07,
    "sm_pool_skip_dst": 1.6296e-06,
    "sm_two_blocks": 2.1064e-06,
    "sm_two_blocks_pool": 9.5318e-07,
    "sm_lowres_2x2": 8.4393e-07,
    "sm_lowres_4x4": 9.9460e-07,
    "sm_lowres_8x8": 1.5156e-06,
    "sm_lowres_10x6": 1.2701e-06,
    "sm_lowres_pool": 1.7511e-06,
    "sm_lowres_two_blocks": 1.6301e-06,
    "sm_lowres_two_blocks_relu0": 2.0457e-06,
    "sm_head1_sig0": 7.7240e-07,
    "sm_head1_sig1": 1.5202e-06,
    "sm_head17_sig0": 9.3556e-07,
    "sm_head17_sig1": 1.3172e-06,
    "sm_head_lowres": 1.2181e-06,
}
# MEASURED-END
