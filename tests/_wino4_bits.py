"""Cases, launch and file names of the F(4x4,3x3) bitwise fixtures (tests/golden/wino4_bits/), shared by tools/gen_wino4_bits_golden.py (which writes them) and
tests/test_gpu_wino4_bits.py (which requires them back bit for bit).

The fixtures are what ``conv3x3_wino4_kernel`` stored for seeded float operands on an MI355X BEFORE its K loop's address and select instructions were hoisted; a change of
that kind moves no floating-point operation, so every output bit stays.  Each case is one ``ph_debug_conv3x3_run`` launch with ``conv_wino4`` = 3, on the operands
``tests/_conv3x3.py`` draws for the case's name.  The smallest shapes at which that code can go wrong:

    plain_16x32          64 -> 64:   one workgroup tile, 16 quarters
    cout96_20x36         64 -> 96:   cut tiles; the last N tile is half empty (its upper waves run the loop without weight loads)
    lowres_16x32/24x40   64 + 64 at half resolution -> 64: the folded bilinear, halo clamps on all four borders; the K loop changes its transform at quarter 16
    pool_skip_dst_16x32  64 -> 64, fused pool, dst not written
    splitk2_16x32        128 -> 64 in two K slices: the split-K instantiation, a slice that starts at quarter 16 and quarters beyond a slice's end
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np
import torch

from tests import _conv3x3 as R

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wino4_bits")
_W4 = (("use_wino4", 3),)

CASES = [
    R.Case("w4bits_plain_16x32", R.K_WINO4, cout=64, cin0=64, H=16, W=32, B=1, opts=_W4),
    R.Case("w4bits_cout96_20x36", R.K_WINO4, cout=96, cin0=64, H=20, W=36, B=1, opts=_W4),
    R.Case("w4bits_lowres_16x32", R.K_WINO4, cout=64, cin0=64, cin1=64, H=16, W=32, B=1, lowres=True, opts=_W4),
    R.Case("w4bits_lowres_24x40", R.K_WINO4, cout=64, cin0=64, cin1=64, H=24, W=40, B=1, lowres=True, opts=_W4),
    R.Case("w4bits_pool_skip_dst_16x32", R.K_WINO4, cout=64, cin0=64, H=16, W=32, B=1, pool=True, skip_dst=True, opts=_W4),
    R.Case("w4bits_splitk2_16x32", R.K_WINO4, cout=64, cin0=128, H=16, W=32, B=1, splitk=2, scratch="fits", ksplit=2, opts=_W4),
]


def golden_path(case) -> str:
    return os.path.join(GOLDEN_DIR, case.name[len("w4bits_"):] + ".npy")


def run(case, n_cu: int) -> np.ndarray:
    """The case's launch on cuda:0 -> what it stored (dst; the pooled tensor where dst is not written), float32; the route's report is asserted."""
    from sleap_nn_amd import _lib as L

    dev = "cuda:0"
    g = R.geometry(case, n_cu)
    o = R.operands(case, "float", n_cu)
    B, H, W = g["B"], g["H"], g["W"]
    src0 = o["src0"].to(dev)
    src1 = o["src1"].to(dev) if case.cin1 else None
    dst = torch.full((B, H, W, g["coutp"]), float("nan"), dtype=torch.float32, device=dev)
    pool = torch.full((B, g["Hp"], g["Wp"], g["coutp"]), float("nan"), dtype=torch.float32, device=dev) if case.pool else None
    scratch = torch.zeros(g["scratch_bytes"] // 4, dtype=torch.float32, device=dev) if case.scratch else None
    weight, bias = o["weight"].contiguous(), o["bias"].contiguous()
    rc = L.ConvRunCase(cin0=case.cin0, cin1=case.cin1, cout=case.cout, bn=g["bn"], B=B, H=H, W=W, forms=g["forms"], flags=g["flags"], head_cout=0, relu=case.relu,
                       splitk_finish=case.splitk_finish, head_sigmoid=0, kernel=-9, kv=-9, ksplit=-9, props=-9, n_cu=-9, counters_zero=-9,
                       split_scratch_bytes=g["scratch_bytes"], src0=src0.data_ptr(), src1=src1.data_ptr() if src1 is not None else None, dst=dst.data_ptr(),
                       dst_pool=pool.data_ptr() if pool is not None else None, relu_mask_src=None, head_dst=None,
                       split_scratch=scratch.data_ptr() if scratch is not None else None, weight=weight.data_ptr(), bias=bias.data_ptr(), head_w=None, head_b=None,
                       **g["options"])
    torch.cuda.synchronize()
    L.check(L.lib().ph_debug_conv3x3_run(C.byref(rc)))
    torch.cuda.synchronize()
    assert (rc.kernel, rc.ksplit) == (R.K_WINO4, case.ksplit), (case.name, "routed to", R.KERNEL_NAMES[rc.kernel], rc.ksplit)
    out = pool if case.skip_dst else dst
    return out.cpu().numpy()
