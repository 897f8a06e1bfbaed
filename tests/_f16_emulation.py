"""The plain-fp16 UNet pipe's arithmetic contract, evaluated in float64 on the CPU, with a derived per-element bound.

The contract (headers of csrc/f16_kernels.hip and csrc/f16_rows_kernels.hip): fp16 operands, fp32 accumulation in some order, bias and ReLU in fp32, ONE
round-to-nearest-even to fp16 wherever a tensor is stored (HBM or LDS), max pool exact, heads in fp32.  ``Emulation.run`` walks a ``Model``'s op program and returns, for
every tensor, a pair ``(r, e)`` of float64 NCHW tensors: ``r`` are the numbers a conforming device stores, ``e >= 0`` is such that every conforming device value ``d``
has ``|d - r| <= e``.  Nothing here is measured; every rule is derived from the kernels' arithmetic:

* network input.  OP_STEM on stem_f16_kernel (``stem_f16mfma`` 1): ``fl16(fl32(x / 255))`` for uint8 frames (f16_kernels.hip: ``sLut[tid] = (_Float16)((float)tid / 255.0f)``),
  ``fl16(x)`` for float frames; e = 0.  Two kernels do NOT round the image to fp16, and the emulation follows them: ``input_conv3x3_kernel`` (net_kernels.hip, the OP_INPUT_CONV
  of a network whose first block is wider than 16 channels: ``v = (float)u8 / 255.0f; acc += v * w`` with the fp32 weights ``a.w``) and ``stem_fused_kernel<CIN, 3>``
  (``stem_f16mfma`` 0: the first conv in fp32 on fp32 weights, "the first conv's fp32 output is rounded to fp16 as it is read").  There the input is ``fl32(x / 255)`` and the
  first conv's weights are the fp32 ones.
* weights of every other 3x3 conv: ``fl16(w)``, round to nearest even (``f16_weight_pack_kernel``: ``split_hi(v) = (_Float16)v``, v_cvt_f16_f32; the stem kernels convert with
  the same cast); biases stay fp32.
* 3x3 conv (+ ReLU) stored as fp16: ``y`` the float64 conv of ``r_in`` with those weights plus bias, ``S`` the same conv of the magnitudes, ``n = 9 Cin + 1``, ``u = 2^-24``,
  ``gamma_n = n u / (1 - n u)``; ``delta = gamma_n S + (1 + gamma_n) conv(|w|, e_in)`` (the fp32 evaluation in any order is within ``gamma_n S_d`` of the exact sum over the DEVICE's
  inputs, ``S_d <= S + conv(|w|, e_in)``: hence the ``1 + gamma_n``); ``r = fl16(relu(y))``, ``e = max |fl16(relu(y +- delta)) - r|`` -- rounding and ReLU are monotone, so ``e`` is 0
  wherever no fp16 midpoint lies within ``delta`` of ``y``.  fp16 subnormals keep their 2^-24 spacing.
* 2x2 max pool, zero padding when odd: ``r`` the max of the window, ``e`` the max of ``e`` over the window.
* bilinear x2, packed-fp16 arithmetic (``upsample_f16math`` 1; ``upsample2x_fmt_kernel`` and ``blend16`` of the row-tile kernel, operation for operation): per axis
  ``fl16(fma(near, 3/4, fl16(far / 4)))``, columns first, border taps clamped.  An fp16 fma is exact in float64 before its rounding, so this is bit-exact (e = 0 when e_in = 0);
  every operation is monotone in the inputs, so for e_in > 0 the same arithmetic on ``r_in - e_in`` and ``r_in + e_in`` brackets the device.
* bilinear x2, fp32 arithmetic (``upsample_f16math`` 0): the float64 blend with ATen's weights rounded once; the conv's delta rule with ``n = 5`` (``hy (hx a + lx b) + ly (hx c + lx d)``:
  the four products by 1/4 or 3/4 of fp16 numbers are exact in fp32, then two inner sums, two outer products and the last sum round).
* 1x1 head, fp32 out: ``e = gamma_n S + (1 + gamma_n) conv(|w|, e_in) + u |y|``.  ``head1x1_mfma_kernel`` holds the fp32 weights (``n = Cin + 1``); the fused epilogues hold each
  weight as ``hi = fl16(w)``, ``lo' = fl16((w - hi) 2048)`` and compute ``hacc + haccx / 2048 + b``: the emulation evaluates with ``hi + lo' / 2048`` itself, so the representation
  error of the pair (at most 2^-22 |w|) is IN ``y`` and no term stands for it; two chains, ``n = 2 Cin + 3``, ``S`` over ``|hi| + |lo'| / 2048``.  Sigmoid: derivative bound 1/4, plus
  ``8 u`` for expf, the sum and the division in fp32 on a value in (0, 1).
* transposed conv: ``conv_transpose2d(stride 2, padding 1, output_padding 1)`` on fp16 weights; the device runs it as a 3x3 conv over the zero-stuffed tensor, so the conv's rule
  holds with the conv's ``n`` (products with the stuffed zeros are exact).

Teacher forcing: ``run(image, forced={slot: device tensor})`` restarts from the device's own values -- every reader of a forced slot sees them with ``e = 0`` -- while the pair
returned FOR that slot is still the prediction from the op's (possibly forced) inputs: what ``check`` compares the device tensor with.

``standin`` is a second, independent evaluation of the same plan in torch fp32 (``conv2d`` on ``.float()`` operands, ``.half()`` at each store): a conforming "device" without a
GPU, with switches that make it subtly wrong (tests/test_f16_emulation_cpu.py).
"""
import math

import torch
import torch.nn.functional as F

from sleap_nn_amd import _lib as L

U32 = 2.0 ** -24  # unit roundoff of fp32


def gamma(n):
    return n * U32 / (1.0 - n * U32)


def round_to(x, bits=11, emin=-14):
    """float64 -> nearest (ties to even) binary float with ``bits`` significand bits and smallest normal 2^emin, subnormals kept; the result stays float64.  (11, -14) is
    fp16.  Written out in float64 because a float64 -> float16 cast may round twice (through fp32)."""
    m, ex = torch.frexp(x)  # x = m 2^ex, 0.5 <= |m| < 1
    q = torch.pow(2.0, (torch.clamp(ex, min=emin + 1) - bits).to(torch.float64))
    r = torch.round(x / q) * q
    return r.clamp(-65504.0, 65504.0) if bits == 11 else r  # (only a bracket y +- delta of a long chain gets here; saturating it keeps the bound finite, and an inf on the device still fails it)


def fl16(x):
    return round_to(x, 11, -14)


def fl32(x):
    return x.to(torch.float32).to(torch.float64)  # (one correctly rounded conversion)


def same_pool(x):
    h, w = x.shape[-2:]
    return F.max_pool2d(F.pad(x, (0, w % 2, 0, h % 2)), 2, 2)  # zeros beyond the image


def _near_far(n_out, n_in):
    o = torch.arange(n_out)
    near = o // 2
    far = torch.where(o % 2 == 1, near + 1, near - 1).clamp(0, n_in - 1)
    return near, far


def upsample_f16math(x, fl):
    """upsample2x_fmt_kernel's packed-fp16 arithmetic: columns first (t = fl(fma(h_near, 3/4, fl(h_far / 4)))), then rows, every rounding where the kernel has one."""
    H, W = x.shape[-2:]
    nx, fx = _near_far(2 * W, W)
    ny, fy = _near_far(2 * H, H)
    t = fl(x[..., :, nx] * 0.75 + fl(x[..., :, fx] * 0.25))
    return fl(t[..., ny, :] * 0.75 + fl(t[..., fy, :] * 0.25))


def upsample_exact(x):
    """ATen's bilinear x2, align_corners=False, in the tensor's own precision: weights 3/4 and 1/4, border taps clamped."""
    H, W = x.shape[-2:]
    nx, fx = _near_far(2 * W, W)
    ny, fy = _near_far(2 * H, H)
    t = x[..., :, nx] * 0.75 + x[..., :, fx] * 0.25
    return t[..., ny, :] * 0.75 + t[..., fy, :] * 0.25


def split_pair(w):
    """The fused head epilogues' weights: hi = fl16(w), lo' = fl16((w - hi) 2048) (act_format.h: split_hi / split_lo on the fp32 weight)."""
    w = fl32(w)
    hi = fl16(w)
    lo = fl16(fl32((w - hi) * 2048.0))
    return hi, lo


def _bracket(y, delta, act, fl):
    r = fl(act(y))
    e = torch.maximum((fl(act(y + delta)) - r).abs(), (fl(act(y - delta)) - r).abs())
    return r, e


def normalized(image):
    """fl32(x / 255) for uint8 frames, the fp32 value for float frames (taken as already normalised), float64 NCHW."""
    if image.dtype == torch.uint8:
        return fl32(image.double() / 255.0)
    return image.to(torch.float32).double()


class Emulation:
    """``model``: a sleap_nn_amd Model on its inference (fused) program; ``sd``: its state dict.  ``rounded=False`` replaces every fl16 / fl32 by the identity (the helper then IS
    oracle.cpu_ref.model_forward in float64).  ``fused_heads``: indices of head ops the device computed in a conv epilogue ((hi, lo') weights), as ``last_kernels()`` reports
    them (PH_KV_FUSED)."""

    def __init__(self, model, sd, rounded=True, upsample_f16math=1, stem_f16mfma=1, fused_heads=()):
        self.ops = list(model.ops)
        self.sd = {k: v.double() for k, v in sd.items()}
        self.rounded = rounded
        self.f16math = bool(upsample_f16math)
        self.stem_f16 = bool(stem_f16mfma)
        self.fused_heads = set(fused_heads)
        self.fl = fl16 if rounded else (lambda x: x)
        self.fl32 = fl32 if rounded else (lambda x: x)

    # ---- the rules
    def conv(self, parts, w, b, relu, n, w_is_f16=True, transposed=False):
        """parts: [(r, e), ...] concatenated along the channels.  -> (r, e) of the stored fp16 tensor."""
        x = torch.cat([p[0] for p in parts], 1)
        ex = torch.cat([p[1] for p in parts], 1)
        w = self.fl(w) if w_is_f16 else self.fl32(w)
        if transposed:
            op = lambda t, ww, bb: F.conv_transpose2d(t, ww, bb, stride=2, padding=1, output_padding=1)
        else:
            op = lambda t, ww, bb: F.conv2d(t, ww, bb, padding=w.shape[-1] // 2)
        y = op(x, w, b)
        act = torch.relu if relu else (lambda t: t)
        if not self.rounded:
            return act(y), torch.zeros_like(y)
        S = op(x.abs(), w.abs(), b.abs())
        g = gamma(n)
        delta = g * S + (1.0 + g) * op(ex, w.abs(), None)
        return _bracket(y, delta, act, self.fl)

    def pool(self, p):
        return same_pool(p[0]), same_pool(p[1])

    def upsample(self, p):
        r_in, e_in = p
        if not self.rounded:
            return upsample_exact(r_in), torch.zeros_like(upsample_exact(r_in))
        if self.f16math:
            r = upsample_f16math(r_in, self.fl)
            if float(e_in.max()) == 0.0:
                return r, torch.zeros_like(r)
            lo, hi = upsample_f16math(r_in - e_in, self.fl), upsample_f16math(r_in + e_in, self.fl)  # every operation is monotone
            return r, torch.maximum(hi - r, r - lo)
        y = upsample_exact(r_in)
        g = gamma(5)
        delta = g * upsample_exact(r_in.abs()) + (1.0 + g) * upsample_exact(e_in)
        return _bracket(y, delta, lambda t: t, self.fl)

    def head(self, p, w, b, sigmoid, fused):
        r_in, e_in = p
        cin = w.shape[1]
        if not self.rounded:
            y = F.conv2d(r_in, w, b)
            return (torch.sigmoid(y) if sigmoid else y), torch.zeros_like(y)
        if fused:
            hi, lo = split_pair(w)
            w_eff, w_abs, n = hi + lo / 2048.0, hi.abs() + lo.abs() / 2048.0, 2 * cin + 3
        else:
            w_eff = fl32(w)
            w_abs, n = w_eff.abs(), cin + 1
        b = fl32(b)
        y = F.conv2d(r_in, w_eff, b)
        g = gamma(n)
        e = g * F.conv2d(r_in.abs(), w_abs, b.abs()) + (1.0 + g) * F.conv2d(e_in, w_abs, None) + U32 * y.abs()
        if sigmoid:
            return torch.sigmoid(y), 0.25 * e + 8 * U32
        return y, e

    # ---- the walk
    def run(self, image, forced=None):
        """-> {("slot", s): (r, e), ("head", out_index): (r, e)}.  ``forced``: {slot: NCHW tensor read back from the device}."""
        forced = {k: v.double().cpu() for k, v in (forced or {}).items()}
        x32 = normalized(image)  # (the oracle normalises in fp32 as well: oracle.cpu_ref.normalize_input)
        val, out = {}, {}
        self.behind_unstored = set()  # keys of tensors computed from an input with e > 0: behind a tensor the device never stored (or, unforced, behind anything)

        def put(slot, pair, sources=()):
            out[("slot", slot)] = pair
            if any(float(s[1].max()) > 0.0 for s in sources):
                self.behind_unstored.add(("slot", slot))
            val[slot] = (forced[slot], torch.zeros_like(forced[slot])) if slot in forced else pair

        zero = torch.zeros_like(x32)
        for i, op in enumerate(self.ops):
            relu = bool(op.flags & L.FLAG_RELU)
            w = self.sd[op.weight] if op.weight else None
            b = self.sd[op.bias] if op.bias else None
            if op.kind == L.OP_INPUT_CONV:  # input_conv3x3_kernel: fp32 image, fp32 weights, one rounding at the store
                put(op.dst, self.conv([(x32, zero)], w, b, relu, op.ksize * op.ksize * op.cin0 + 1, w_is_f16=False))
            elif op.kind == L.OP_STEM:
                first_in = self.fl(x32) if self.stem_f16 else x32
                mid = self.conv([(first_in, zero)], w, b, True, 9 * op.cin0 + 1, w_is_f16=self.stem_f16)  # the halo tile in LDS: stored once, as fp16
                full = self.conv([mid], self.sd[op.weight2], self.sd[op.bias2], relu, 9 * op.cmid + 1)
                out[("stem_mid", i)] = mid
                if op.dst >= 0:
                    put(op.dst, full, [mid])
                    put(op.dst2, self.pool(val[op.dst]), [val[op.dst]])  # (the kernel pools its own registers: under teacher forcing those are the forced full-resolution values)
                else:
                    put(op.dst2, self.pool(full), [mid])
            elif op.kind == L.OP_CONV:
                parts = [val[op.src0]] + ([val[op.src1]] if op.src1 >= 0 else [])
                put(op.dst, self.conv(parts, w, b, relu, op.ksize * op.ksize * (op.cin0 + op.cin1) + 1), parts)
                if op.dst2 >= 0:
                    put(op.dst2, self.pool(val[op.dst]), [val[op.dst]])
            elif op.kind == L.OP_POOL:
                put(op.dst, self.pool(val[op.src0]), [val[op.src0]])
            elif op.kind == L.OP_UPSAMPLE:
                put(op.dst, self.upsample(val[op.src0]), [val[op.src0]])
            elif op.kind == L.OP_CONVT:
                put(op.dst, self.conv([val[op.src0]], w, b, relu, 9 * op.cin0 + 1, transposed=True), [val[op.src0]])
            elif op.kind == L.OP_HEAD:
                assert not (op.flags & L.FLAG_SOFTMAX), "class-vector heads run exact: not part of the plain-fp16 pipe"
                out[("head", op.out_index)] = self.head(val[op.src0], w, b, bool(op.flags & L.FLAG_SIGMOID), i in self.fused_heads)
            else:
                raise NotImplementedError(f"op kind {op.kind} is not part of the plain-fp16 UNet pipe")
        return out


def check(device, r, e):
    """-> (worst |d - r| - e over the tensor: <= 0 means inside the bound, share of elements with d != r, worst |d - r| / e where e > 0 or 0.0)."""
    d = device.double().cpu()
    assert d.shape == r.shape, (d.shape, r.shape)
    diff = (d - r).abs()
    pos = e > 0
    ratio = float((diff[pos] / e[pos]).max()) if bool(pos.any()) else 0.0
    return float((diff - e).max()), float((d != r).double().mean()), ratio


# ---------------------------------------------------------------------------------------------------------------------------------------------
# The stand-in device: the same storage plan in torch fp32
# ---------------------------------------------------------------------------------------------------------------------------------------------
MUTATIONS = ("truncate_store", "fp16_chunk_sums", "bias_after_rounding", "bilinear_last_row_tap", "double_rounded_intermediate", "right_border_tap_dropped")


def _trunc_half(t):
    """fp32 -> fp16 toward zero (the mutation; a conforming store rounds to nearest even)."""
    h = t.half()
    over = h.float().abs() > t.abs()
    bits = h.view(torch.int16)
    return torch.where(over, (bits - 1).view(torch.float16), h)  # one step toward zero (sign-magnitude: the same decrement of the pattern for either sign)


def standin(model, sd, image, upsample_f16math=1, stem_f16mfma=1, fused_heads=(), mutation=None, forced=None):
    """-> {("slot", s): fp32 tensor holding fp16 values, ("stem_mid", i): ..., ("head", k): fp32}: what a conforming device would leave, computed with torch fp32
    ``conv2d`` on ``.float()`` operands and ``.half()`` at every store.  ``mutation``: one of MUTATIONS, or None."""
    assert mutation is None or mutation in MUTATIONS, mutation
    forced = {k: v.float().cpu() for k, v in (forced or {}).items()}
    sd = {k: v.float() for k, v in sd.items()}
    x32 = (image.float() / 255.0) if image.dtype == torch.uint8 else image.float()
    store = (lambda t: _trunc_half(t).float()) if mutation == "truncate_store" else (lambda t: t.half().float())
    val, out = {}, {}

    def put(slot, t):
        out[("slot", slot)] = t
        val[slot] = forced.get(slot, t)

    def conv(x, w, b, relu, f16w=True, transposed=False, intermediate=False):
        w = w.half().float() if f16w else w
        if transposed:
            op = lambda t, ww, bb: F.conv_transpose2d(t, ww, bb, stride=2, padding=1, output_padding=1)
        else:
            op = lambda t, ww, bb: F.conv2d(t, ww, bb, padding=w.shape[-1] // 2)
        if mutation == "fp16_chunk_sums" and not transposed:
            y = sum(op(x[:, c : c + 32], w[:, c : c + 32], None).half().float() for c in range(0, x.shape[1], 32)) + b.view(1, -1, 1, 1)
        elif mutation == "bias_after_rounding":
            y = op(x, w, None).half().float() + b.view(1, -1, 1, 1)
        else:
            y = op(x, w, b)
        if mutation == "right_border_tap_dropped" and not transposed and w.shape[-1] == 3:
            wt = torch.zeros_like(w)
            wt[:, :, 1, 0] = w[:, :, 1, 0]  # the tap to the left of the centre, missing at x = W - 1 only
            y[..., -1] -= F.conv2d(x, wt, None, padding=1)[..., -1]
        y = torch.relu(y) if relu else y
        if mutation == "double_rounded_intermediate" and intermediate:
            y = y.bfloat16().float()
        return store(y)

    def up(x):
        if upsample_f16math:
            H, W = x.shape[-2:]
            nx, fx = _near_far(2 * W, W)
            ny, fy = _near_far(2 * H, H)
            if mutation == "bilinear_last_row_tap":
                fy = fy.clone()
                fy[-1] = max(H - 2, 0)  # the last row's second tap clamped one pixel early
            h = x.half()
            c75, c25 = torch.tensor(0.75).half(), torch.tensor(0.25).half()
            fma = lambda a, q: fl16(a.double() * 0.75 + q.double()).half()  # (an fp16 fma: exact in float64 before its one rounding)
            t = fma(h[..., :, nx], (h[..., :, fx] * c25))
            return fma(t[..., ny, :], (t[..., fy, :] * c25)).float()
        H, W = x.shape[-2:]
        nx, fx = _near_far(2 * W, W)
        ny, fy = _near_far(2 * H, H)
        if mutation == "bilinear_last_row_tap":
            fy = fy.clone()
            fy[-1] = max(H - 2, 0)
        t = x[..., :, nx] * 0.75 + x[..., :, fx] * 0.25
        return store(t[..., ny, :] * 0.75 + t[..., fy, :] * 0.25)

    for i, op in enumerate(model.ops):
        relu = bool(op.flags & L.FLAG_RELU)
        w = sd[op.weight] if op.weight else None
        b = sd[op.bias] if op.bias else None
        if op.kind == L.OP_INPUT_CONV:
            put(op.dst, conv(x32, w, b, relu, f16w=False))
        elif op.kind == L.OP_STEM:
            mid = conv(x32.half().float() if stem_f16mfma else x32, w, b, True, f16w=bool(stem_f16mfma), intermediate=True)
            out[("stem_mid", i)] = mid
            full = conv(mid, sd[op.weight2], sd[op.bias2], relu)
            if op.dst >= 0:
                put(op.dst, full)
                put(op.dst2, same_pool(val[op.dst]))
            else:
                put(op.dst2, same_pool(full))
        elif op.kind == L.OP_CONV:
            x = torch.cat([val[op.src0]] + ([val[op.src1]] if op.src1 >= 0 else []), 1)
            nxt = model.ops[i + 1] if i + 1 < len(model.ops) else None
            inter = nxt is not None and nxt.kind == L.OP_CONV and nxt.src0 == op.dst and nxt.src1 < 0 and op.dst2 < 0  # the first conv of a block: what block2_c32_f16_kernel keeps in LDS
            put(op.dst, conv(x, w, b, relu, intermediate=inter))
            if op.dst2 >= 0:
                put(op.dst2, same_pool(val[op.dst]))
        elif op.kind == L.OP_POOL:
            put(op.dst, same_pool(val[op.src0]))
        elif op.kind == L.OP_UPSAMPLE:
            put(op.dst, up(val[op.src0]))
        elif op.kind == L.OP_CONVT:
            put(op.dst, conv(val[op.src0], w, b, relu, transposed=True))
        elif op.kind == L.OP_HEAD:
            x = val[op.src0]
            if i in fused_heads:
                hi, lo = split_pair(w.double())
                y = F.conv2d(x, hi.float(), None) + F.conv2d(x, lo.float(), None) * (1.0 / 2048.0) + b.view(1, -1, 1, 1)
            else:
                y = F.conv2d(x, w, b)
            out[("head", op.out_index)] = torch.sigmoid(y) if op.flags & L.FLAG_SIGMOID else y
        else:
            raise NotImplementedError(op.kind)
    return out
