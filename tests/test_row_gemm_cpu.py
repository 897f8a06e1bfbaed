"""The float64 reference of the row-GEMM tests (tests/_row_gemm.py) held to independent formulations, and the conditions its case table rests on.  No GPU."""
import torch
import torch.nn.functional as F

from tests import _row_gemm as R

SMALL = [c for c in R.CASES if R.geometry(c)["in_rows"] <= 4096]


def _sources(c, g, o):
    x = R._nchw(o["src0"], g["B"], g["H"], g["W"], c.cin0)
    return torch.cat([x, R._nchw(o["src1"], g["B"], g["H"], g["W"], c.cin1)], 1) if c.cin1 else x


def _by_taps(c, g, x, w):
    """Modes 0, 1, 2, 5, 6 as the kernel's comment states them: a sum over taps of (shifted, zero-filled, strided pixels) x (that tap's (cout, cin) matrix)."""
    k = {0: 1, 1: 2, 2: 3, 5: c.ksize, 6: 1}[c.mode]
    stride = {0: 1, 1: 2, 2: 1, 5: 1, 6: c.tap_stride}[c.mode]
    pad = 0 if c.mode == 1 else k // 2
    B, cin, H, W = x.shape
    OH, OW = (H // stride, W // stride)
    xp = torch.zeros(B, cin, H + 2 * pad + k, W + 2 * pad + k, dtype=x.dtype)
    xp[:, :, pad : pad + H, pad : pad + W] = x
    y = torch.zeros(B, c.cout, OH, OW, dtype=x.dtype)
    for ky in range(k):
        for kx in range(k):
            sl = xp[:, :, ky : ky + stride * OH : stride, kx : kx + stride * OW : stride]
            y += torch.einsum("bchw,oc->bohw", sl, w[:, :, ky * k + kx])
    return y


def test_run_entry_is_declared_and_bound():
    import ctypes as C
    import os
    import re

    from sleap_nn_amd import _lib as L

    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "posehip.h")).read()
    assert "int ph_debug_gemm_run(ph_gemm_case* c);" in header and int(re.search(r"^#define\s+PH_VERSION\s+(\d+)", header, re.M).group(1)) >= 129
    fields = re.search(r"typedef struct ph_gemm_case \{(.*?)\} ph_gemm_case;", header, re.S).group(1)
    names = [n.strip(" *") for decl in fields.split(";") if decl.strip() for n in decl.split(",")]
    names = [n.split()[-1].strip("*") for n in names]
    assert names == [n for n, _ in L.GemmCase._fields_]
    assert L.lib().ph_gemm_case_size() == C.sizeof(L.GemmCase)


def test_tap_modes_equal_a_sum_over_taps():
    seen = set()
    for c in SMALL:
        if c.mode in (0, 1, 2, 5, 6) and not c.out_patch:
            g = R.geometry(c)
            o = R.operands(c, "float")
            acc, written = R.linear_part(c, g, o)
            y = _by_taps(c, g, _sources(c, g, o), o["weight"].to(torch.float64))
            assert bool(written.all()) and torch.allclose(acc, R._rows(y, g["coutp"]), rtol=0, atol=1e-12), c.name
            seen.add(c.mode)
    assert seen == {0, 1, 2, 5, 6}


def test_transposed_conv_phases_equal_zero_stuffing_and_a_3x3_conv():
    n = 0
    for c in SMALL:
        if c.mode != 3:
            continue
        g = R.geometry(c)
        o = R.operands(c, "float")
        acc, written = R.linear_part(c, g, o)
        x = _sources(c, g, o)
        B, cin, H, W = x.shape
        z = torch.zeros(B, cin, 2 * H + 2, 2 * W + 2, dtype=x.dtype)  # zero-stuffed, one pixel of padding in front, two behind (padding 1, output_padding 1)
        z[:, :, 1 : 2 * H : 2, 1 : 2 * W : 2] = x
        wc = o["weight"].to(torch.float64).flip(2, 3).permute(1, 0, 2, 3)  # (cout, cin, 3, 3), taps flipped
        y = R._rows(F.conv2d(z, wc), g["coutp"])
        assert torch.allclose(acc[written], y[written], rtol=0, atol=1e-12), c.name
        ph = torch.zeros(B, 1, 2 * H, 2 * W, dtype=torch.bool)
        if c.all_phases:
            ph[:] = True
        else:
            ph[:, :, c.out_tap >> 1 :: 2, c.out_tap & 1 :: 2] = True
        assert torch.equal(written, R._rows(ph, 1)[:, 0]), c.name
        n += 1
    assert n >= 10


def test_stride2_conv_equals_a_same_conv_subsampled():
    n = 0
    for c in SMALL:
        if c.mode != 4:
            continue
        g = R.geometry(c)
        o = R.operands(c, "float")
        acc, _ = R.linear_part(c, g, o)
        full = F.conv2d(_sources(c, g, o), o["weight"].to(torch.float64).reshape(c.cout, c.cin0 + c.cin1, 3, 3), padding=1)
        assert torch.allclose(acc, R._rows(full[:, :, ::2, ::2], g["coutp"]), rtol=0, atol=1e-12), c.name
        n += 1
    assert n >= 4


def test_out_patch_taps_are_the_data_gradient_of_the_patch_conv():
    """Four Linear launches, tap t with weight Wf[:, :, ty, tx]^T and scattered to (2 oy + ty, 2 ox + tx), assemble autograd's gradient of Conv2d(k2, s2)."""
    cases = [c for c in R.CASES if c.mode == 0 and c.out_patch and c.name.startswith("patchconv_dgrad_3x5")]
    assert sorted(c.out_tap for c in cases) == [0, 1, 2, 3]
    c0 = cases[0]
    g = R.geometry(c0)
    gen = torch.Generator().manual_seed(3)
    wf = torch.rand(c0.cin0, c0.cout, 2, 2, generator=gen, dtype=torch.float64) - 0.5  # the forward conv: cout -> cin0 channels (the GEMM's roles swapped)
    o = R.operands(c0, "float")
    gy = R._nchw(o["src0"], g["B"], g["H"], g["W"], c0.cin0)
    x = torch.zeros(g["B"], c0.cout, g["out_H"], g["out_W"], dtype=torch.float64, requires_grad=True)
    (F.conv2d(x, wf, stride=2) * gy).sum().backward()
    total = torch.zeros(g["out_rows"], g["coutp"], dtype=torch.float64)
    count = torch.zeros(g["out_rows"], dtype=torch.int64)
    for c in cases:
        oc = dict(o, weight=wf[:, :, c.out_tap >> 1, c.out_tap & 1].t().contiguous().reshape(c.cout, c.cin0, 1))
        acc, written = R.linear_part(c, g, oc)
        total[written] += acc[written]
        count += written
    assert bool((count == 1).all())
    assert torch.allclose(total, R._rows(x.grad, g["coutp"]), rtol=0, atol=1e-12)


def test_act3_is_the_gradient_through_gelu():
    c = R.BY_NAME["epi1_act3_alone"]
    o = R.operands(c, "float")
    ref = R.reference(c, o)
    aux = o["aux"].to(torch.float64).requires_grad_(True)
    (F.gelu(aux) * ref["pre"]).sum().backward()
    assert torch.allclose(ref["dst"], aux.grad, rtol=0, atol=1e-12)
    z = torch.linspace(-6, 6, 1001, dtype=torch.float64, requires_grad=True)
    F.silu(z).sum().backward()
    zs = z.detach()
    assert torch.allclose(R.silu64(zs), F.silu(zs), rtol=0, atol=1e-15) and torch.allclose(R.gelu64(zs), F.gelu(zs), rtol=0, atol=1e-15)
    assert float(z.grad.abs().max()) <= R.ACT_LIPSCHITZ["silu"]
    z2 = zs.clone().requires_grad_(True)
    F.gelu(z2).sum().backward()
    assert float(z2.grad.abs().max()) <= R.ACT_LIPSCHITZ["gelu"] and torch.allclose(R.gelu_grad64(zs), z2.grad, rtol=0, atol=1e-14)


def test_epilogue_forms_follow_the_documented_order():
    """act(acc + bias) * scale + residual; act(scale * (acc + bias) + shift); act(acc + bias + residual) for the one-tap strided mode; pad channels: scale 0 + residual."""
    for name, f in (("pair_v0_persist0_1", None), ("convt_3x5_all_affine1", None), ("tap1_6x10_s2_res1_act1", None), ("n_bn96_cout72", None)):
        c = R.BY_NAME[name]
        g = R.geometry(c)
        o = R.operands(c, "float")
        ref = R.reference(c, o)
        acc, _ = R.linear_part(c, g, o)
        n = c.cout
        a = acc[:, :n] + o["bias"].to(torch.float64)
        res = o["residual"][:, :n].to(torch.float64) if c.residual else 0.0
        act = {0: lambda v: v, 1: lambda v: v.clamp(min=0), 2: R.gelu64, 4: R.silu64}[c.act]
        if c.mode == 6:
            want = act(a + res)
        elif c.affine_first:
            want = act(o["scale"].to(torch.float64) * a + o["shift"].to(torch.float64))
        else:
            want = act(a) * (o["scale"].to(torch.float64) if c.scale else 1.0) + res
        assert torch.allclose(ref["dst"][:, :n], want, rtol=0, atol=1e-12), name
        pad = ref["dst"][:, n:]
        if pad.numel():
            want_pad = o["residual"][:, n:].to(torch.float64) if c.residual else torch.zeros_like(pad)
            assert torch.equal(pad, act(want_pad) if c.mode == 6 else want_pad), name


def test_sums_of_squares_follow_blocks_and_samples():
    for hw in (6, 40, 256):
        c = R.BY_NAME[f"epi2_sumsq_hw{hw}_linear"]
        g = R.geometry(c)
        ref = R.reference(c, R.operands(c, "exact"))
        sq, d = ref["sumsq"], ref["dst"]
        # summed over the blocks and places that belong to one sample, the partials are the sample's sum of squares
        per_sample = torch.zeros(g["M"] // hw, g["coutp"], dtype=torch.float64)
        for b in range(sq.shape[0]):
            for s in range(sq.shape[1]):
                if not torch.isnan(sq[b, s, 0]):
                    per_sample[32 * b // hw + s] += sq[b, s]
        assert torch.equal(per_sample, (d * d).reshape(g["M"] // hw, hw, -1).sum(1)), hw
        assert g["sq_nseg"] == 31 // hw + 2


def test_exact_family_is_exact():
    """max S < 2^24 for every case: every partial sum of the exact operands is an fp32 integer (a half-integer under scale 0.5), in any order."""
    worst = 0.0
    for c in R.CASES:
        g = R.geometry(c)
        bound = (16.0 * (c.cin0 + c.cin1) * (9 if c.mode == 3 else g["taps"]) + 4.0) * 2.0 + 4.0  # |a|, |w| <= 4, |bias|, |residual|, |shift| <= 4, |scale| <= 2
        if g["in_rows"] <= 4096:
            ref = R.reference(c, R.operands(c, "exact"))
            assert float(ref["S"].max()) <= bound, c.name
            assert bool((ref["dst"] * 2 == (ref["dst"] * 2).round()).all()) or not c.linear, c.name
        worst = max(worst, bound)
    assert worst < 2.0 ** 24 / 100


def test_cout_values_yield_the_intended_n_tile():
    want = {128: (128, 240, 384, 120), 96: (96, 80, 288, 72), 64: (64, 48, 320, 56), 32: (32, 16, 144, 160, 136)}
    for bn, couts in want.items():
        for cout in couts:
            assert R.choose_bn(R.pad16(cout)) == bn, (bn, cout)
            assert R.geometry(R.BY_NAME[f"n_bn{bn}_cout{cout}"])["bn"] == bn
        tails = [R.pad16(c) % bn == 0 for c in couts]
        assert True in tails and False in tails and any(R.pad16(c) > 2 * bn for c in couts) and any(c % 16 for c in couts)
    for c in R.CASES:  # an explicit variant goes with its N tile
        g = R.geometry(c)
        assert R.VARIANT_BN[g["variant"]] == g["bn"], c.name
    assert R.geometry(R.BY_NAME["choice_variant4"])["variant"] == 4 and R.geometry(R.BY_NAME["choice_variant0"])["variant"] == 0


def test_the_table_is_complete_and_notices_a_missing_case():
    assert R.missing_coverage(R.CASES) == []
    for v in range(5):
        for tmpl in R.TEMPLATES:
            gone = [c for c in R.CASES if c.name != f"pair_v{v}_{tmpl}_0"]
            assert len(gone) == len(R.CASES) - 1 and ("pair", v, tmpl) in R.missing_coverage(gone), (v, tmpl)
    k = [R.geometry(c) for c in R.CASES if "k" in c.tags]
    assert {g["c0p"] for g in k if not g["c1p"]} >= {16, 32, 48, 96, 112} and {(g["c0p"], g["c1p"]) for g in k if g["c1p"]} == {(16, 48), (48, 16)}
    assert {g["nstages"] % 3 for g in k} == {0, 1, 2}
    for n_cu in (256, 304, 64):  # the persistent cases leave their first tile behind on any chip
        multi = [R.geometry(c, n_cu) for c in R.CASES if "persist" in c.tags]
        assert all(g["mtiles"] * g["ntc"] > n_cu for g in multi) and {g["mtiles"] % 8 == 0 for g in multi} == {True, False}
