"""Reference, operands and case table of the row-GEMM tests (csrc/convnext_kernels.hip: gemm_mfma_dma_kernel, the persistent kernel, and gemm_mfma_dma_tile_kernel;
DESIGN.md K23), shared by tests/test_row_gemm_cpu.py and tests/test_gpu_row_gemm.py.

Reference: float64, plain torch ops.  The linear part of every mode is one ``F.conv2d`` / ``F.conv_transpose2d`` on NCHW tensors of the TRUE channel counts; the epilogue
follows in the padded row layout the kernel stores, as ``GemmArgs`` (csrc/net_kernels.h) documents it.  Beside the value the reference returns, per output element, the
sum of magnitudes S = (sum_k |a_k| |w_k| + |bias|) |scale| + |residual| (mode 6 and affine-first: the same terms where their epilogue has them) the error bound is built on.

Two operand families:
  exact   integers in [-4, 4] (scale from {0.5, 1, 2}): every partial sum in any order is an fp32 integer (or half-integer) while max S < 2^24, so a linear epilogue must
          come out EQUAL to the reference.  max S < 2^24 is a condition of the test (test_row_gemm_cpu.py asserts it for every exact case), not a measurement.
  float   uniform in [-0.5, 0.5).  Linear epilogues: |d - r| <= gamma_n S, n = K + 3 (K products of the row, each rounded at most once as a product and K - 1 times in
          the accumulation in whatever order, then the bias add, the scale and the residual add), gamma_n = n u / (1 - n u), u = 2^-24.  Through an activation f the
          error of the argument passes with f's Lipschitz constant and the device function adds its own error, c_f u |x|: see ``ACT_BAR``.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field, replace
from typing import Callable, Optional, Union

import torch
import torch.nn.functional as F

U = 2.0 ** -24
NAN = float("nan")
VARIANT_TM = {0: 256, 1: 256, 2: 256, 3: 256, 4: 128}
VARIANT_BN = {0: 128, 1: 96, 2: 64, 3: 32, 4: 128}
BN_VARIANTS = {128: (0, 4), 96: (1,), 64: (2,), 32: (3,)}
GUARD_ROWS = 8  # NaN rows before and after every device tensor
CHIP_CUS = 256  # the constant of launch_gemm's variant rule (an MI355X; the persistent grid itself is sized by the device's own count)

# The device activations' own error, |f_device(x) - f(x)| <= c u |x| for GELU (gelu_f) and SiLU, |g'_device(z) - g'(z)| <= c u for the GELU derivative (gelu_grad_f):
# c = twice the worst value an MI355X gave over every case of the table (the margin tests/test_gpu_f16_emulation.py gives a measured bar), measured between two launches
# that differ in `act` alone, so that the argument is the device's own fp32 pre-activation.  DESIGN.md (K23, "Held to float64 at the tile edges") has the measured values.
ACT_MEASURED = {"gelu": 5.0868, "silu": 1.7956, "gelu_grad": 4.5125}
ACT_BAR = {k: (None if v is None else 2.0 * v) for k, v in ACT_MEASURED.items()}
ACT_LIPSCHITZ = {"gelu": 1.13, "silu": 1.10}  # sup |gelu'| = 1.1290, sup |silu'| = 1.0998


def pad16(c: int) -> int:
    return (c + 15) // 16 * 16


def gamma(n: int) -> float:
    return n * U / (1.0 - n * U)


def choose_bn(coutp: int) -> int:
    """gemm_choose_bn restated: the N tile that pads coutp least, the larger tile on a tie."""
    best, best_pad = 128, 1 << 30
    for bn in (128, 96, 64, 32):
        padded = (coutp + bn - 1) // bn * bn
        if padded < best_pad:
            best, best_pad = bn, padded
    return best


def choose_variant(M: int, coutp: int, bn: int) -> int:
    """launch_gemm's rule restated."""
    if bn != 128:
        return {96: 1, 64: 2, 32: 3}[bn]
    nt = (coutp + 127) // 128
    b0, b4 = (M + 255) // 256 * nt, (M + 127) // 128 * nt
    e0 = b0 / ((b0 + CHIP_CUS - 1) // CHIP_CUS * CHIP_CUS)
    e4 = 0.95 * b4 / ((b4 + CHIP_CUS - 1) // CHIP_CUS * CHIP_CUS)
    return 4 if e4 > e0 else 0


@dataclass(frozen=True)
class Case:
    name: str
    mode: int
    cout: int
    cin0: int
    cin1: int = 0
    variant: int = -1                       # -1: launch_gemm's own choice (asserted against choose_variant)
    bn: int = 0                             # 0: gemm_choose_bn's own choice (asserted against choose_bn)
    M: Union[int, Callable[[int], int]] = 0  # mode 0 without out_patch: rows, possibly a function of the CU count
    B: int = 3
    H: Union[int, Callable[[int], int]] = 0  # the INPUT map (mode 0 + out_patch: the map of the rows)
    W: Union[int, Callable[[int], int]] = 0
    ksize: int = 0
    tap_stride: int = 1
    out_patch: int = 0
    out_tap: int = 0
    all_phases: int = 0
    act: int = 0                            # 0 none, 1 ReLU, 2 GELU, 3 times GELU'(aux), 4 SiLU
    scale: bool = False
    residual: bool = False
    affine_first: bool = False              # scale and shift before the activation
    dst_pre: bool = False
    sq_hw: int = 0
    late_split: int = 0
    persist2: int = 0
    tags: tuple = field(default_factory=tuple)

    @property
    def linear(self) -> bool:
        return self.act in (0, 1)

    @property
    def template(self) -> str:
        """Which kernel template launch_gemm_variant dispatches this case to."""
        if self.mode == 0:
            return "persist0_epi1" if (self.act == 3 or self.dst_pre) else ("persist0_epi2" if self.sq_hw else "persist0")
        if self.mode == 1:
            return "persist1"
        if self.mode == 2:
            return "persist2" if self.persist2 else "tile2"
        return f"tile{self.mode}"

    @property
    def epilogue(self) -> frozenset:
        forms = {{0: "bias", 1: "relu", 2: "gelu", 3: "act3", 4: "silu"}[self.act]}
        if self.mode == 6 and self.residual:
            forms = {"residual_before_relu" if self.act == 1 else "residual_before_none"}
        elif self.affine_first:
            forms.add("affine_first")
        elif self.scale and self.residual:
            forms.add("scale_residual")
        if self.dst_pre:
            forms.add("dst_pre")
        if self.sq_hw:
            forms.add("sumsq")
        if self.out_patch and self.mode != 3:
            forms.add("out_patch")
        return frozenset(forms)


TEMPLATES = ("persist0", "persist0_epi1", "persist0_epi2", "persist1", "persist2", "tile2", "tile3", "tile4", "tile5", "tile6")
EPILOGUES = ("bias", "relu", "gelu", "scale_residual", "affine_first", "silu", "residual_before_relu", "act3", "dst_pre", "sumsq", "out_patch")


def geometry(c: Case, n_cu: int = CHIP_CUS) -> dict:
    """Sizes of a case on a chip of n_cu CUs: rows, maps, taps, stages, the expected N tile and variant."""
    H = c.H(n_cu) if callable(c.H) else c.H
    W = c.W(n_cu) if callable(c.W) else c.W
    g = {"H": H, "W": W, "out_H": 0, "out_W": 0}
    if c.mode == 0 and not c.out_patch:
        M = c.M(n_cu) if callable(c.M) else c.M
        g.update(B=1, H=M, W=1, M=M, in_rows=M, out_rows=M, taps=1)  # (the reference sees the rows as an M x 1 map)
    elif c.mode == 0:  # data gradient of a 2x2/stride-2 conv: rows (b, oy, ox) scattered to (2 oy + ty, 2 ox + tx)
        M = c.B * H * W
        g.update(B=c.B, M=M, in_rows=M, out_rows=4 * M, taps=1, out_H=2 * H, out_W=2 * W)
    elif c.mode in (1, 4):
        M = c.B * (H // 2) * (W // 2)
        g.update(B=c.B, M=M, in_rows=c.B * H * W, out_rows=M, taps=4 if c.mode == 1 else 9)
    elif c.mode in (2, 5):
        M = c.B * H * W
        g.update(B=c.B, M=M, in_rows=M, out_rows=M, taps=9 if c.mode == 2 else c.ksize * c.ksize)
    elif c.mode == 3:
        M = c.B * H * W
        g.update(B=c.B, M=M, in_rows=M, out_rows=4 * M, taps=9, out_H=2 * H, out_W=2 * W)
    else:
        M = c.B * (H // c.tap_stride) * (W // c.tap_stride)
        g.update(B=c.B, M=M, in_rows=c.B * H * W, out_rows=M, taps=1)
    coutp = pad16(c.cout)
    bn = c.bn or choose_bn(coutp)
    variant = c.variant if c.variant >= 0 else choose_variant(M, coutp, bn)
    slices = (pad16(c.cin0) + 31) // 32 + ((pad16(c.cin1) + 31) // 32 if c.cin1 else 0)
    ktaps = g["taps"] if c.mode != 3 else (9 if c.all_phases else (1 + (c.out_tap >> 1)) * (1 + (c.out_tap & 1)))
    g.update(coutp=coutp, c0p=pad16(c.cin0), c1p=pad16(c.cin1) if c.cin1 else 0, bn=bn, variant=variant, TM=VARIANT_TM[variant], ntc=(coutp + bn - 1) // bn,
             mtiles=(M + VARIANT_TM[variant] - 1) // VARIANT_TM[variant], K=(c.cin0 + c.cin1) * (4 if (c.mode == 3 and c.all_phases) else ktaps),
             nstages=slices * (ktaps if not (c.mode == 3 and c.all_phases) else 4))  # (all_phases: the stages of the 4-tap phase; K: the most products any phase sums)
    g["sq_nseg"] = (31 // c.sq_hw + 2) if c.sq_hw else 0
    return g


# ---- operands

def _draw(gen, shape, family):
    if family == "exact":
        return torch.randint(-4, 5, shape, generator=gen).to(torch.float32)
    return torch.rand(shape, generator=gen, dtype=torch.float32) - 0.5


def _padded_rows(t, cp):
    out = torch.zeros(t.shape[0], cp, dtype=t.dtype)
    out[:, : t.shape[1]] = t
    return out


def operands(c: Case, family: str, n_cu: int = CHIP_CUS, seed: int = 0) -> dict:
    """CPU float32 tensors: the sources as padded NHWC rows (pad channels zero), the canonical weight / bias / scale / shift, residual and aux in the output's row layout
    (every padded channel drawn: the pad channels of the output must come out as scale 0 + residual)."""
    g = geometry(c, n_cu)
    gen = torch.Generator().manual_seed(1000 + seed + sum(map(ord, c.name)))
    cin = c.cin0 + c.cin1
    o = {"src0": _padded_rows(_draw(gen, (g["in_rows"], c.cin0), family), g["c0p"])}
    o["src1"] = _padded_rows(_draw(gen, (g["in_rows"], c.cin1), family), g["c1p"]) if c.cin1 else None
    o["weight"] = _draw(gen, (cin, c.cout, 3, 3) if c.mode == 3 else (c.cout, cin, g["taps"]), family)
    o["bias"] = _draw(gen, (c.cout,), family)
    o["scale"] = o["shift"] = o["residual"] = o["aux"] = None
    if c.scale or c.affine_first:
        o["scale"] = (2.0 ** torch.randint(-1, 2, (c.cout,), generator=gen).to(torch.float32)) if family == "exact" else _draw(gen, (c.cout,), family) * 4.0
    if c.affine_first:
        o["shift"] = _draw(gen, (c.cout,), family)
    if c.residual:
        o["residual"] = _draw(gen, (g["out_rows"], g["coutp"]), family)
    if c.act == 3:
        o["aux"] = _draw(gen, (g["out_rows"], g["coutp"]), "float") * 6.0  # the GELU derivative over [-3, 3)
    return o


# ---- reference

def _nchw(rows, B, H, W, c):
    return rows[:, :c].to(torch.float64).reshape(B, H, W, c).permute(0, 3, 1, 2)


def _rows(nchw, cp):
    B, c, H, W = nchw.shape
    return _padded_rows(nchw.permute(0, 2, 3, 1).reshape(B * H * W, c), cp)


def gelu64(x):
    return 0.5 * x * (1.0 + torch.erf(x * math.sqrt(0.5)))


def gelu_grad64(x):
    return 0.5 * (1.0 + torch.erf(x * math.sqrt(0.5))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


def silu64(x):
    return x / (1.0 + torch.exp(-x))


def _conv(c: Case, g: dict, x, w):
    """The linear part of mode c.mode on NCHW float64 `x` (both sources concatenated) and the canonical weight -> (B, cout, OH, OW) on the output grid of the rows."""
    cin = c.cin0 + c.cin1
    if c.mode == 0:
        return F.conv2d(x, w.reshape(c.cout, cin, 1, 1))
    if c.mode == 1:
        return F.conv2d(x, w.reshape(c.cout, cin, 2, 2), stride=2)
    if c.mode == 2:
        return F.conv2d(x, w.reshape(c.cout, cin, 3, 3), padding=1)
    if c.mode == 3:
        return F.conv_transpose2d(x, w, stride=2, padding=1, output_padding=1)
    if c.mode == 4:
        return F.conv2d(x, w.reshape(c.cout, cin, 3, 3), stride=2, padding=1)
    if c.mode == 5:
        return F.conv2d(x, w.reshape(c.cout, cin, c.ksize, c.ksize), padding=c.ksize // 2)
    return F.conv2d(x, w.reshape(c.cout, cin, 1, 1), stride=c.tap_stride)


def linear_part(c: Case, g: dict, o: dict, magnitudes: bool = False):
    """(acc, written): acc = (out_rows, coutp) float64 product sums in the output's row layout -- of the magnitudes if asked --, written = bool per output row."""
    x = _nchw(o["src0"], g["B"], g["H"], g["W"], c.cin0)
    if c.cin1:
        x = torch.cat([x, _nchw(o["src1"], g["B"], g["H"], g["W"], c.cin1)], 1)
    w = o["weight"].to(torch.float64)
    y = _conv(c, g, x.abs() if magnitudes else x, w.abs() if magnitudes else w)
    written = torch.ones(y.shape[0], 1, y.shape[2], y.shape[3], dtype=torch.bool)
    if c.mode == 3 and not c.all_phases:  # one phase of the transposed conv: the other three are not this launch's
        written[:] = False
        written[:, :, c.out_tap >> 1 :: 2, c.out_tap & 1 :: 2] = True
    elif c.mode != 3 and c.out_patch:  # each row's result lands on pixel (2 oy + ty, 2 ox + tx) of the out_H x out_W map
        full = torch.zeros(y.shape[0], y.shape[1], g["out_H"], g["out_W"], dtype=y.dtype)
        full[:, :, c.out_tap >> 1 :: 2, c.out_tap & 1 :: 2] = y
        written = torch.zeros(y.shape[0], 1, g["out_H"], g["out_W"], dtype=torch.bool)
        written[:, :, c.out_tap >> 1 :: 2, c.out_tap & 1 :: 2] = True
        y = full
    assert y.shape[0] * y.shape[2] * y.shape[3] == g["out_rows"], (c.name, y.shape, g)
    return _rows(y, g["coutp"]), _rows(written, 1)[:, 0]


def _vec(v, cp):
    out = torch.zeros(cp, dtype=torch.float64)
    if v is not None:
        out[: v.numel()] = v.to(torch.float64)
    return out


def reference(c: Case, o: dict, n_cu: int = CHIP_CUS) -> dict:
    """-> dst, bound (float family: the a-priori bound per element; None where ACT_BAR is still to be measured), S, written (rows), pre (the activation's argument),
    dst_pre, sumsq / sumsq_bound ((blocks, sq_nseg, coutp), NaN where the launch writes nothing)."""
    g = geometry(c, n_cu)
    cp = g["coutp"]
    acc, written = linear_part(c, g, o)
    mag, _ = linear_part(c, g, o, magnitudes=True)
    bias = _vec(o["bias"], cp)
    scale = _vec(o["scale"], cp) if o["scale"] is not None else None  # zero-padded, as the packers pad it
    shift = _vec(o["shift"], cp)
    res = o["residual"].to(torch.float64) if o["residual"] is not None else torch.zeros_like(acc)
    gn = gamma(g["K"] + 3)
    pre, s_pre = acc + bias, mag + bias.abs()
    post = torch.ones(cp, dtype=torch.float64)
    if c.mode == 6:
        pre, s_pre = pre + res, s_pre + res.abs()
        res = torch.zeros_like(acc)
    elif c.affine_first:
        pre, s_pre = scale * pre + shift, scale.abs() * s_pre + shift.abs()
    elif scale is not None:
        post = scale
    out = {"written": written, "pre": pre, "dst_pre": None, "sumsq": None, "sumsq_bound": None}
    act_err = None  # the device activation's own error, in units of its (measured) bar
    if c.act == 0:
        f, lip = pre, 1.0
    elif c.act == 1:
        f, lip = pre.clamp(min=0.0), 1.0
    elif c.act == 2:
        f, lip, act_err = gelu64(pre), ACT_LIPSCHITZ["gelu"], ("gelu", pre.abs())
    elif c.act == 4:
        f, lip, act_err = silu64(pre), ACT_LIPSCHITZ["silu"], ("silu", pre.abs())
    else:
        aux = o["aux"].to(torch.float64)
        gp = gelu_grad64(aux)
        f, lip, act_err = pre * gp, gp.abs(), ("gelu_grad", pre.abs())
    dst = f * post + res
    out["dst"] = dst
    out["S"] = s_pre * post.abs() + res.abs()
    if c.linear:
        out["bound"] = gn * out["S"]
    elif ACT_BAR[act_err[0]] is None:
        out["bound"] = None
    else:  # argument within gn s_pre; through f; f's own error; then the product with the scale, the residual add (and act 3's own product): three more roundings
        out["bound"] = (lip * gn * s_pre + ACT_BAR[act_err[0]] * U * act_err[1]) * post.abs() + gamma(3) * ((f * post).abs() + res.abs())
    if c.dst_pre:
        out["dst_pre"] = o["aux"].to(torch.float64) if c.act == 3 else pre
        out["dst_pre_bound"] = torch.zeros_like(pre) if c.act == 3 else gn * s_pre
    if c.sq_hw:  # per 32-row block and sample segment (first sample of the block + segment): the sum of dst^2 over the block's rows of that sample
        nblk, nseg = (g["M"] + 31) // 32, g["sq_nseg"]
        sq = torch.full((nblk, nseg, cp), NAN, dtype=torch.float64)
        sb = None if out["bound"] is None else torch.full((nblk, nseg, cp), NAN, dtype=torch.float64)
        for b in range(nblk):
            r0, r1 = 32 * b, min(32 * b + 32, g["M"])
            for sg in range(r0 // c.sq_hw, (r1 - 1) // c.sq_hw + 1):
                lo, hi = max(r0, sg * c.sq_hw), min(r1, (sg + 1) * c.sq_hw)
                v = dst[lo:hi]
                sq[b, sg - r0 // c.sq_hw] = (v * v).sum(0)
                if sb is not None:  # the squares of values within e of v, summed over <= 32 rows by a five-level tree: seven roundings
                    e = out["bound"][lo:hi]
                    hi2 = ((v.abs() + e) ** 2).sum(0)
                    sb[b, sg - r0 // c.sq_hw] = (2.0 * v.abs() * e + e * e).sum(0) + gamma(7) * hi2
        out["sumsq"], out["sumsq_bound"] = sq, sb
    return out


# ---- the case table: the smallest shapes that reach each edge

def _m_persist_rows(n_cu):  # (2 n_cu + 3) tiles of 256 rows, the last one five rows short: every workgroup walks a third tile, some a partial one
    return (2 * n_cu + 3) * 256 - 5


def _m_tiles8(n_cu):  # the first multiple of 8 above n_cu M tiles (the XCD dealing's branch), each with three N tiles
    return ((n_cu + 1 + 7) // 8 * 8) * 256


def _side_persist(n_cu):  # a square map whose batch of 3 makes more than n_cu / 3 M tiles of 256 rows (x 3 N tiles: past the CU count), mtiles no multiple of 8
    side = 2
    while True:
        mt = (3 * side * side + 255) // 256
        if mt * 3 > n_cu and mt % 8:
            return side
        side += 2


def _m_variant4(n_cu):  # 128-row tiles fill the chip's last round better: launch_gemm takes variant 4
    return 128 * 3


def _m_variant0(n_cu):  # 256-row tiles fill a whole round of the chip: variant 0
    return 256 * CHIP_CUS


def _table():
    t = []
    add = t.append
    # -- every (variant, template) pair, with the M, N and K edges dealt over them
    n_of = {128: (128, 240, 384, 120), 96: (96, 80, 288, 72), 64: (64, 48, 320, 56), 32: (32, 16, 144, 160, 136)}
    k_of = ((16, 0), (32, 0), (48, 0), (96, 0), (112, 0), (13, 40), (40, 13))  # c0p 16 (one stage + the dummy), 32, 48, 96, 112; two sources (16, 48) and (48, 16)
    i = 0
    for v in range(5):
        TM, bn = VARIANT_TM[v], VARIANT_BN[v]
        m_of = (1, TM - 1, TM, TM + 1)
        for tmpl in TEMPLATES:
            for rep in range(2):  # two cases per pair: the completeness test must notice when ONE goes missing
                cout = n_of[bn][i % len(n_of[bn])]
                cin0, cin1 = k_of[i % len(k_of)]
                kw = dict(variant=v, cout=cout, cin0=cin0, cin1=cin1, tags=("pair",))
                name = f"pair_v{v}_{tmpl}_{rep}"
                if tmpl.startswith("persist0"):
                    M = m_of[i % 4]
                    if tmpl == "persist0":
                        add(Case(name, 0, M=M, act=(0, 1, 2, 0)[i % 4], scale=i % 4 == 3, residual=i % 4 == 3, **kw))
                    elif tmpl == "persist0_epi1":
                        add(Case(name, 0, M=M, act=3 if rep else 2, dst_pre=True, **kw))
                    else:
                        hw = (6, 40)[rep]
                        add(Case(name, 0, M=(M + hw - 1) // hw * hw, act=2 * rep, sq_hw=hw, **kw))
                elif tmpl == "persist1":
                    add(Case(name, 1, H=(2, 6)[rep], W=(2, 10)[rep], act=rep, **kw))
                elif tmpl in ("persist2", "tile2"):
                    add(Case(name, 2, H=(3, 7)[rep], W=(5, 9)[rep], act=rep, persist2=int(tmpl == "persist2"), **kw))
                elif tmpl == "tile3":
                    kw.update(cin0=cin0 + cin1, cin1=0)
                    add(Case(name, 3, H=3, W=5, out_patch=1, out_tap=i % 4, all_phases=rep, act=4 * rep, affine_first=bool(rep), **kw))
                elif tmpl == "tile4":
                    add(Case(name, 4, H=(2, 6)[rep], W=(2, 10)[rep], act=(1, 4)[rep], affine_first=bool(rep), **kw))
                elif tmpl == "tile5":
                    add(Case(name, 5, H=3, W=4, ksize=(5, 3)[rep], act=rep, **kw))
                else:
                    kw.update(cin0=cin0 + cin1, cin1=0)
                    add(Case(name, 6, H=6, W=10, tap_stride=1 + rep, act=1, residual=True, **kw))
                i += 1
    # -- launch_gemm's own choice between variants 0 and 4
    add(Case("choice_variant4", 0, cout=128, cin0=32, M=_m_variant4, tags=("choice",)))
    add(Case("choice_variant0", 0, cout=128, cin0=16, M=_m_variant0, tags=("choice",)))
    # -- N: per N tile one full tile, a partial last tile, three or more tiles, and a true cout that is no multiple of 16
    for bn, couts in n_of.items():
        for cout in couts:
            add(Case(f"n_bn{bn}_cout{cout}", 0, cout=cout, cin0=48, M=257, scale=True, residual=True, tags=("n",)))
    # -- K: every slice count, half-empty slices, two sources with channel counts that are no multiple of 16
    for cin0, cin1 in ((16, 0), (32, 0), (48, 0), (96, 0), (112, 0), (13, 40), (40, 13), (5, 0)):
        add(Case(f"k_{cin0}_{cin1}", 0, cout=48, cin0=cin0, cin1=cin1, M=300, tags=("k",)))
        add(Case(f"k9_{cin0}_{cin1}", 2, cout=48, cin0=cin0, cin1=cin1, H=7, W=9, tags=("k",)))
    # -- M at the tile edges of both tile heights
    for v in (0, 4):
        TM = VARIANT_TM[v]
        for M in (1, TM - 1, TM, TM + 1):
            add(Case(f"m_v{v}_{M}", 0, variant=v, cout=128, cin0=32, M=M, act=1, tags=("m",)))
    # -- the persistent kernel past its first tile
    add(Case("persist_rows", 0, variant=3, cout=16, cin0=16, M=_m_persist_rows, act=1, tags=("persist",)))               # ntc = 1, one stage + the dummy stage
    add(Case("persist_rows_k48", 0, variant=3, cout=32, cin0=48, M=_m_persist_rows, scale=True, residual=True, tags=("persist",)))  # two stages: the ring phase moves on per tile
    add(Case("persist_ntc3_tiles8", 0, variant=3, bn=32, cout=96, cin0=16, cin1=16, M=_m_tiles8, tags=("persist", "late")))  # mtiles % 8 == 0: the XCD dealing
    add(Case("persist_ntc3_epi1", 0, variant=3, bn=32, cout=96, cin0=32, M=_m_tiles8, act=2, dst_pre=True, tags=("persist",)))
    add(Case("persist_ntc3_epi2", 0, variant=3, bn=32, cout=96, cin0=32, M=_m_tiles8, sq_hw=256, tags=("persist",)))
    add(Case("persist_mode1", 1, variant=3, bn=32, cout=96, cin0=16, H=lambda n: 2 * _side_persist(n), W=lambda n: 2 * _side_persist(n), act=1, tags=("persist",)))  # four stages
    add(Case("persist_mode2", 2, variant=3, bn=32, cout=96, cin0=16, H=_side_persist, W=_side_persist, persist2=1, tags=("persist",)))  # nine stages
    # -- spatial modes, batch 3: tiles straddle images
    for H, W in ((1, 1), (2, 2), (3, 5), (7, 9)):
        for p2 in (0, 1):
            add(Case(f"conv3_{H}x{W}_persist{p2}", 2, cout=40, cin0=24, cin1=8, H=H, W=W, persist2=p2, act=1, tags=("spatial",)))
    for H, W in ((2, 2), (6, 10)):
        add(Case(f"s2conv3_{H}x{W}", 4, cout=144, cin0=72, H=H, W=W, act=1, tags=("spatial",)))  # three 32-channel slices under nine taps, five N tiles of 32
        add(Case(f"s2conv3_{H}x{W}_bn128", 4, cout=240, cin0=40, H=H, W=W, tags=("spatial",)))  # two slices, two N tiles of 128, the second partial
        add(Case(f"patchconv_{H}x{W}", 1, cout=80, cin0=24, H=H, W=W, tags=("spatial",)))
        for tap in range(4):  # the data gradient of that conv: one Linear launch per tap, scattered
            add(Case(f"patchconv_dgrad_{H // 2}x{W // 2}_tap{tap}", 0, cout=24, cin0=80, H=H // 2, W=W // 2, out_patch=1, out_tap=tap, tags=("spatial",)))
        for stride in (1, 2):
            for res in (False, True):
                for act in (0, 1):
                    add(Case(f"tap1_{H}x{W}_s{stride}_res{int(res)}_act{act}", 6, cout=240, cin0=40, H=H, W=W, tap_stride=stride, residual=res, act=act, tags=("spatial",)))
    for H, W in ((1, 1), (3, 5)):
        for affine in (False, True):
            for tap in range(4):
                add(Case(f"convt_{H}x{W}_phase{tap}_affine{int(affine)}", 3, cout=40, cin0=24, H=H, W=W, out_patch=1, out_tap=tap, affine_first=affine, act=4 if affine else 0, tags=("spatial",)))
            add(Case(f"convt_{H}x{W}_all_affine{int(affine)}", 3, cout=40, cin0=24, H=H, W=W, out_patch=1, all_phases=1, affine_first=affine, act=4 if affine else 1, tags=("spatial",)))
    for k in (1, 5, 7, 9):
        for H, W in ((3, 4), (9, 11)):
            add(Case(f"conv{k}_{H}x{W}", 5, cout=24, cin0=8, cin1=8 if k == 5 else 0, H=H, W=W, ksize=k, act=1, tags=("spatial",)))
    # -- the training epilogues and the sums of squares
    add(Case("epi1_act3", 0, cout=80, cin0=40, M=300, act=3, dst_pre=True, scale=True, residual=True, tags=("epi",)))
    add(Case("epi1_act3_alone", 0, cout=80, cin0=40, M=300, act=3, tags=("epi",)))
    add(Case("epi1_gelu_pre", 0, cout=80, cin0=40, M=300, act=2, dst_pre=True, tags=("epi",)))
    for hw in (6, 40, 256):
        add(Case(f"epi2_sumsq_hw{hw}", 0, cout=80, cin0=40, M={6: 300, 40: 280, 256: 512}[hw], act=2, sq_hw=hw, tags=("epi",)))
        add(Case(f"epi2_sumsq_hw{hw}_linear", 0, cout=80, cin0=40, M={6: 300, 40: 280, 256: 512}[hw], sq_hw=hw, tags=("epi",)))
    return t


CASES = _table()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES), "case names must be unique"
LATE_SPLIT_CASE = "persist_ntc3_tiles8"  # run under late_split 0, 1, 2: the accumulation order does not depend on it


def with_late_split(c: Case, late_split: int) -> Case:
    return replace(c, late_split=late_split)


def missing_coverage(cases) -> list:
    """What a table must reach and `cases` does not: every (variant, template) pair launch_gemm_variant can dispatch, every mode, every epilogue form, and per N tile a
    full and a partial last tile."""
    missing = []
    have = {}
    for c in cases:
        if "pair" in c.tags:  # the cases that are in the table for their pair's sake
            have.setdefault((geometry(c)["variant"], c.template), []).append(c.name)
    for v in range(5):
        for tmpl in TEMPLATES:
            if len(have.get((v, tmpl), [])) < 2:  # two, so that one case of a pair cannot leave the table unnoticed
                missing.append(("pair", v, tmpl))
    for mode in range(7):
        if not any(c.mode == mode for c in cases):
            missing.append(("mode", mode))
    forms = set().union(*(c.epilogue for c in cases)) if cases else set()
    missing += [("epilogue", e) for e in EPILOGUES if e not in forms]
    for bn in (128, 96, 64, 32):
        tails = {geometry(c)["coutp"] % bn == 0 for c in cases if geometry(c)["bn"] == bn}
        missing += [("n tile", bn, "full" if full else "partial") for full in (True, False) if full not in tails]
    return missing
