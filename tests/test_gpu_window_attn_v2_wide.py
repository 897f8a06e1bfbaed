"""The key-tiled cosine window attention kernel (csrc/swinv2_kernels.hip: window_attn_v2_wide_kernel) alone: one launch through ``ph_debug_window_attn_v2_wide_run`` on
tensors the test owns, against the float64 NumPy statement of tests/_swinv2_cases.py (which tests/test_pretrained_swinv2_wide_cpu.py ties to HuggingFace's layer at
windows 12 and 16).

The bound is the one tests/test_gpu_window_attn_v2.py gives the one-wave kernel: per case, FOUR times the error of the reference's own fp32 evaluation of the same
operation against float64 (tests/_swinv2_wide_cases.hf_order_fp32: torch on the CPU, HuggingFace's order, the mask added twice).  The online softmax adds one rounding
per moved maximum to each accumulator; the forced-rescale cases make the maximum move where random operands seldom do.  Measured figures are in DESIGN 4.4i."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import _swinv2_cases as SC
from tests import _swinv2_wide_cases as WC

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def run_kernel(qkv, bias, scale, table, heads, w, shift):
    from sleap_nn_amd import _lib as L

    B, H, W = qkv.shape[:3]
    dev = [torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in (qkv, bias, scale, table)]
    dst = torch.full((B, H, W, 32 * heads), float("nan"), dtype=torch.float32, device=DEV)
    torch.cuda.synchronize()
    L.check(L.lib().ph_debug_window_attn_v2_wide_run(*[C.c_void_p(t.data_ptr()) for t in dev], C.c_void_p(dst.data_ptr()), B, H, W, heads, w, shift))
    return dst.cpu().numpy()


@pytest.mark.parametrize("case", WC.KERNEL_CASES, ids=WC.case_id)
def test_kernel_is_within_four_times_the_fp32_reference_error(case):
    w, shift, B, H, W, heads, _clamp, _zero = case
    qkv, bias, scale, table = WC.operands(case)
    want = SC.window_attn_v2_f64(qkv, bias, scale, table, heads, w, shift)
    ref_err = float(np.abs(WC.hf_order_fp32(qkv, bias, scale, table, heads, w, shift).astype(np.float64) - want).max())
    got = run_kernel(qkv, bias, scale, table, heads, w, shift)
    assert got.shape == want.shape and np.isfinite(got).all()  # every pixel of the map is written (the output was NaN-filled)
    err = float(np.abs(got.astype(np.float64) - want).max())
    print(f"w {w} shift {shift} {B}x{H}x{W} heads {heads}: kernel {err:.3g}, fp32 reference {ref_err:.3g}, ratio {err / ref_err:.2f} (scale of the output {np.abs(want).max():.3g})")
    assert ref_err > 0 and err <= 4 * ref_err


@pytest.mark.parametrize("w", [16, 24])
def test_forced_rescale(w):
    """A data-dependent rescale needs an input that forces it: bounded random operands seldom move the maximum far.  Query A's best key sits in the LAST key tile (the maximum jumps by about the scale, 30, after
    every other tile went into the accumulators); query B's maximum rises at every tile.  The same bound on the whole map, and each chosen row against FOUR times the
    reference's error ON THAT ROW (a map-wide maximum can hide one row).  Query A's output is one value row almost exactly, so the reference's error on it can be
    arbitrarily small; the row bound therefore has a floor of one rounding of the stored fp32 output, 2^-24 of the row's largest magnitude, which no fp32 result can
    be asked to beat."""
    (qkv, bias, scale, table), (ta, tb) = WC.forced_rescale_operands(w)
    want = SC.window_attn_v2_f64(qkv, bias, scale, table, 1, w, 0)
    ref = WC.hf_order_fp32(qkv, bias, scale, table, 1, w, 0).astype(np.float64)
    got = run_kernel(qkv, bias, scale, table, 1, w, 0).astype(np.float64)
    assert np.isfinite(got).all()
    ref_err, err = float(np.abs(ref - want).max()), float(np.abs(got - want).max())
    print(f"forced rescale w {w}: kernel {err:.3g}, fp32 reference {ref_err:.3g}, ratio {err / ref_err:.2f}")
    assert ref_err > 0 and err <= 4 * ref_err
    for name, t in (("A", ta), ("B", tb)):
        y, x = divmod(t, w)
        row_ref, row_err = float(np.abs(ref[0, y, x] - want[0, y, x]).max()), float(np.abs(got[0, y, x] - want[0, y, x]).max())
        print(f"  query {name} (token {t}): kernel {row_err:.3g}, fp32 reference of the row {row_ref:.3g}, of the map {ref_err:.3g}")
        floor = 2.0 ** -24 * float(np.abs(want[0, y, x]).max())
        assert row_err <= 4 * max(row_ref, floor), (name, row_err, row_ref, floor)
    # query A's output is its aligned key's value, nearly: the weight of the last token is 1 - O(N e^-30)
    assert float(np.abs(want[0, ta // w, ta % w] - qkv[0, w - 1, w - 1, 64:96]).max()) < 1e-6


@pytest.mark.parametrize("case", [(16, 8, 2, 20, 36, 2, True, True), (9, 4, 2, 10, 19, 3, False, False), (24, 12, 2, 30, 25, 1, False, False)], ids=WC.case_id)
def test_two_launches_are_bit_identical_and_a_batch_of_one_is_its_slice(case):
    w, shift, B, H, W, heads = case[:6]
    qkv, bias, scale, table = WC.operands(case)
    first = run_kernel(qkv, bias, scale, table, heads, w, shift)
    again = run_kernel(qkv, bias, scale, table, heads, w, shift)
    assert np.array_equal(first, again)
    for b in range(B):
        one = run_kernel(qkv[b:b + 1], bias, scale, table, heads, w, shift)
        assert np.array_equal(one, first[b:b + 1]), b


def test_launch_checks_come_back_as_errors():
    from sleap_nn_amd import _lib as L

    t = torch.zeros(1 << 12, dtype=torch.float32, device=DEV)
    p = C.c_void_p(t.data_ptr())
    lib = L.lib()
    assert lib.ph_debug_window_attn_v2_wide_run(p, p, p, p, p, 1, 4, 4, 1, 25, 0) != 0 and "window_size" in lib.ph_last_error().decode()
    assert lib.ph_debug_window_attn_v2_wide_run(p, p, p, p, p, 1, 4, 4, 1, 1, 0) != 0 and "window_size" in lib.ph_last_error().decode()
    assert lib.ph_debug_window_attn_v2_wide_run(p, p, p, p, p, 1, 4, 4, 1, 12, 12) != 0 and "shift" in lib.ph_last_error().decode()
    assert lib.ph_debug_window_attn_v2_wide_run(p, p, p, p, None, 1, 4, 4, 1, 12, 0) != 0 and "null pointer" in lib.ph_last_error().decode()
    assert lib.ph_debug_window_attn_v2_wide_run(p, p, p, p, p, 1, 4, 4, 0, 12, 0) != 0 and "heads" in lib.ph_last_error().decode()
