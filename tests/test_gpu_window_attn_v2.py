"""The cosine window attention kernel (csrc/swin_kernels.hip: window_attn_kernel, cosine variant) alone: one launch through ``ph_debug_window_attn_v2_run`` on tensors the test
owns, against the float64 NumPy statement of tests/_swinv2_cases.py (which tests/test_pretrained_swinv2_cpu.py ties to HuggingFace's layer through tests/swinv2_ref.py).

The bound is the margin tests/test_gpu_conv3x3.py gives the Winograd kernels: per case, FOUR times the error of the reference's own fp32 evaluation of the same operation
against float64 -- torch on the CPU, fp32 tensors, HuggingFace's order of operations (normalize, product, scale, bias, mask added twice, softmax, product).  The margin
covers the hardware exponential and the different summation order; a wrong mask, bias index or norm is an error of order one.  Measured figures are in DESIGN 4.4h."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import _swinv2_cases as SC
from tests import swinv2_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"

# (window, shift, B, H, W, heads, head at the scale clamp, an all-zero token inside the map)
CASES = [
    (2, 0, 2, 5, 7, 1, False, False), (2, 1, 2, 5, 7, 3, True, True),
    (4, 0, 2, 5, 9, 3, False, True), (4, 2, 2, 5, 9, 1, True, False), (4, 2, 2, 8, 12, 3, False, False),
    (7, 0, 2, 9, 15, 1, True, False), (7, 3, 2, 9, 15, 3, False, True), (7, 3, 1, 7, 7, 1, False, False),
    (8, 0, 2, 8, 8, 3, False, False), (8, 4, 2, 8, 8, 1, True, True), (8, 4, 2, 13, 9, 3, True, False),
]


def operands(case):
    w, shift, B, H, W, heads, clamp, zero = case
    g = np.random.default_rng([w, shift, H, W, heads])
    Cc = 32 * heads
    qkv = g.standard_normal((B, H, W, 3 * Cc)).astype(np.float32)
    qkv[..., :Cc] *= g.uniform(0.2, 3.0, size=(B, H, W, 1)).astype(np.float32)  # token norms differ: a missing normalisation shows
    if zero:
        qkv[B - 1, H // 2, W // 2, :] = 0.0  # q = k = v = 0: its normalised k is 0 / 1e-12 = 0
    bias = (0.5 * g.standard_normal(3 * Cc)).astype(np.float32)
    bias[Cc:2 * Cc] = 0.0  # key has no bias: a padded token's k is exactly 0
    scale = g.uniform(5.0, 30.0, size=heads).astype(np.float32)
    if clamp:
        scale[heads - 1] = 100.0
    table = (16.0 / (1.0 + np.exp(-2.0 * g.standard_normal((heads, (2 * w - 1) ** 2))))).astype(np.float32)
    return qkv, bias, scale, table


def hf_order_fp32(qkv, bias, scale, table, heads, w, shift):
    """The same operation in torch on the CPU, fp32, in the order of Swinv2Layer / Swinv2SelfAttention.forward (on a qkv map: a padded token's q, k, v are ``bias``)."""
    x = torch.from_numpy(qkv)
    B, H, W, C3 = x.shape
    Cc = C3 // 3
    pH, pW = -(-H // w) * w, -(-W // w) * w
    full = torch.from_numpy(bias).expand(B, pH, pW, C3).clone()
    full[:, :H, :W] = x
    if shift > 0:
        full = torch.roll(full, shifts=(-shift, -shift), dims=(1, 2))
    win = R.partition(full, w).view(-1, w * w, C3)
    Bn, N = win.shape[0], w * w
    q, k, v = (win[..., i * Cc:(i + 1) * Cc].reshape(Bn, N, heads, 32).transpose(1, 2) for i in range(3))
    s = F.normalize(q, dim=-1) @ F.normalize(k, dim=-1).transpose(-2, -1)
    s = s * torch.from_numpy(scale).view(heads, 1, 1)
    s = s + torch.from_numpy(table)[:, R.position_index(w).view(-1)].view(heads, N, N).unsqueeze(0)
    mask = R.shift_mask(pH, pW, w, shift, torch.float32)
    if mask is not None:
        nm = mask.shape[0]
        s = s.view(Bn // nm, nm, heads, N, N) + mask.unsqueeze(1).unsqueeze(0)
        s = s + mask.unsqueeze(1).unsqueeze(0)
        s = s.view(-1, heads, N, N)
    ctx = (F.softmax(s, dim=-1) @ v).permute(0, 2, 1, 3).contiguous().view(Bn, N, Cc)
    y = R.reverse(ctx.view(-1, w, w, Cc), w, pH, pW)
    if shift > 0:
        y = torch.roll(y, shifts=(shift, shift), dims=(1, 2))
    return y[:, :H, :W].contiguous().numpy()


def run_kernel(case, qkv, bias, scale, table):
    from sleap_nn_amd import _lib as L

    w, shift, B, H, W, heads = case[:6]
    dev = [torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in (qkv, bias, scale, table)]
    dst = torch.full((B, H, W, 32 * heads), float("nan"), dtype=torch.float32, device=DEV)
    torch.cuda.synchronize()
    L.check(L.lib().ph_debug_window_attn_v2_run(*[C.c_void_p(t.data_ptr()) for t in dev], C.c_void_p(dst.data_ptr()), B, H, W, heads, w, shift))
    return dst.cpu().numpy()


@pytest.mark.parametrize("case", CASES, ids=lambda c: "w%d_s%d_b%d_%dx%d_h%d%s%s" % (c[:6] + ("_clamp" if c[6] else "", "_zero" if c[7] else "")))
def test_kernel_is_within_four_times_the_fp32_reference_error(case):
    w, shift, B, H, W, heads, _clamp, _zero = case
    qkv, bias, scale, table = operands(case)
    want = SC.window_attn_v2_f64(qkv, bias, scale, table, heads, w, shift)
    ref_err = float(np.abs(hf_order_fp32(qkv, bias, scale, table, heads, w, shift).astype(np.float64) - want).max())
    got = run_kernel(case, qkv, bias, scale, table)
    assert got.shape == want.shape and np.isfinite(got).all()  # every pixel of the map is written (the output was NaN-filled)
    err = float(np.abs(got.astype(np.float64) - want).max())
    print(f"w {w} shift {shift} {B}x{H}x{W} heads {heads}: kernel {err:.3g}, fp32 reference {ref_err:.3g}, ratio {err / ref_err:.2f} (scale of the output {np.abs(want).max():.3g})")
    assert ref_err > 0 and err <= 4 * ref_err


def test_the_statement_sees_mask_norm_and_padded_keys():
    """What the bound would hide if the float64 statement ignored it: each of these changes the statement by order one (CPU arithmetic; kept with the cases it guards)."""
    case = (4, 2, 2, 5, 9, 1, True, False)
    qkv, bias, scale, table = operands(case)
    base = SC.window_attn_v2_f64(qkv, bias, scale, table, 1, 4, 2)
    assert np.abs(SC.window_attn_v2_f64(qkv, bias, scale, table, 1, 4, 0) - base).max() > 1e-2           # the shift and its band mask
    assert np.abs(SC.window_attn_v2_f64(qkv * 2.0, bias, scale, table, 1, 4, 2) - 2.0 * base).max() > 1e-2  # padded tokens do not scale with the map: they are keys
    assert np.abs(SC.window_attn_v2_f64(qkv, bias, scale, np.roll(table, 1, axis=1), 1, 4, 2) - base).max() > 1e-2  # the bias index
    half = qkv.copy()
    half[..., :32] *= 0.5  # q is normalised: halving it changes nothing
    assert np.abs(SC.window_attn_v2_f64(half, bias, scale, table, 1, 4, 2) - base).max() < 1e-9


def test_launch_checks_come_back_as_errors():
    from sleap_nn_amd import _lib as L

    t = torch.zeros(1 << 12, dtype=torch.float32, device=DEV)
    p = C.c_void_p(t.data_ptr())
    lib = L.lib()
    assert lib.ph_debug_window_attn_v2_run(p, p, p, p, p, 1, 4, 4, 1, 9, 0) != 0 and "window_size" in lib.ph_last_error().decode()
    assert lib.ph_debug_window_attn_v2_run(p, p, p, p, p, 1, 4, 4, 1, 4, 4) != 0 and "shift" in lib.ph_last_error().decode()
    assert lib.ph_debug_window_attn_v2_run(p, p, p, p, None, 1, 4, 4, 1, 4, 0) != 0
