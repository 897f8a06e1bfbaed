"""The row GEMM (csrc/convnext_kernels.hip: gemm_mfma_dma_kernel, gemm_mfma_dma_tile_kernel) called directly through ph_debug_gemm_run on operands the
test owns, against the float64 reference of tests/_row_gemm.py, over its case table: every tile variant, mode and epilogue form at the tile edges.  Per case:

(a) exact operands (small integers): a linear epilogue -- and every ``dst_pre`` -- must EQUAL the reference;
(b) float operands: |d - r| <= the a-priori bound, per element (``_row_gemm.reference``); the sums of squares to their own bound;
(c) every tensor the launch writes lies between NaN guard rows in a NaN-filled buffer: the guards, the rows of the other three phases under ``out_patch`` and the
    sum-of-squares places of samples a block does not touch stay NaN, everything the reference defines is finite.  The sources lie between NaN guards too: a tap that
    reads outside its image shows as a NaN in the output;
(d) the N tile and the variant the library reports are those of the restated rules.

A non-linear case runs a second launch with ``act`` 0: the device's own pre-activation, against which the device activation is held to its bar alone."""
import ctypes as C

import pytest
import torch

from sleap_nn_amd import _lib as L
from tests import _row_gemm as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_WORST = {}  # (mode, what) -> worst error / bound over the cases run so far


def _n_cu():
    return torch.cuda.get_device_properties(0).multi_processor_count


class _Guarded:
    """rows x cp floats between GUARD_ROWS NaN rows on either side, on the device."""

    def __init__(self, rows, cp, fill=None):
        self.rows, self.cp = rows, cp
        self.buf = torch.full((rows + 2 * R.GUARD_ROWS, cp), R.NAN, dtype=torch.float32, device=DEV)
        if fill is not None:
            self.buf[R.GUARD_ROWS : R.GUARD_ROWS + rows] = fill.to(DEV)

    @property
    def ptr(self):
        return self.buf.data_ptr() + R.GUARD_ROWS * self.cp * 4

    def guards_intact(self):
        return bool(torch.isnan(self.buf[: R.GUARD_ROWS]).all()) and bool(torch.isnan(self.buf[R.GUARD_ROWS + self.rows :]).all())

    def body(self):
        return self.buf[R.GUARD_ROWS : R.GUARD_ROWS + self.rows].cpu()


def _launch(case, o, n_cu):
    """One ph_debug_gemm_run -> {"dst", "dst_pre", "sumsq": CPU tensors or None}, the reported (variant, N tile)."""
    g = R.geometry(case, n_cu)
    src0 = _Guarded(g["in_rows"], g["c0p"], o["src0"])
    src1 = _Guarded(g["in_rows"], g["c1p"], o["src1"]) if case.cin1 else None
    res = _Guarded(g["out_rows"], g["coutp"], o["residual"]) if o["residual"] is not None else None
    aux = _Guarded(g["out_rows"], g["coutp"], o["aux"]) if o["aux"] is not None else None
    outs = {"dst": _Guarded(g["out_rows"], g["coutp"])}
    outs["dst_pre"] = _Guarded(g["out_rows"], g["coutp"]) if case.dst_pre else None
    outs["sumsq"] = _Guarded((g["M"] + 31) // 32 * g["sq_nseg"], g["coutp"]) if case.sq_hw else None
    host = {k: (o[k].contiguous() if o[k] is not None else None) for k in ("weight", "bias", "scale", "shift")}
    gc = L.GemmCase(variant=case.variant, mode=case.mode, M=g["M"], H=0 if (case.mode == 0 and not case.out_patch) else g["H"], W=0 if (case.mode == 0 and not case.out_patch) else g["W"],
                    ksize=case.ksize, tap_stride=case.tap_stride, out_patch=case.out_patch, out_tap=case.out_tap, out_H=g["out_H"], out_W=g["out_W"], all_phases=case.all_phases,
                    act=case.act, affine_first=int(case.affine_first), late_split=case.late_split, persist2=case.persist2, sq_hw=case.sq_hw, sq_nseg=g["sq_nseg"],
                    cin0=case.cin0, cin1=case.cin1, cout=case.cout, bn=case.bn, variant_used=-9, bn_used=-9,
                    src0=src0.ptr, src1=src1.ptr if src1 else None, residual=res.ptr if res else None, aux=aux.ptr if aux else None,
                    dst=outs["dst"].ptr, dst_pre=outs["dst_pre"].ptr if outs["dst_pre"] else None, sumsq=outs["sumsq"].ptr if outs["sumsq"] else None,
                    weight=host["weight"].data_ptr(), bias=host["bias"].data_ptr(), scale=host["scale"].data_ptr() if host["scale"] is not None else None,
                    shift=host["shift"].data_ptr() if host["shift"] is not None else None)
    torch.cuda.synchronize()
    L.check(L.lib().ph_debug_gemm_run(C.byref(gc)))
    for k, t in outs.items():
        assert t is None or t.guards_intact(), (case.name, k, "a guard row was written")
    for k, t in (("src0", src0), ("src1", src1), ("residual", res), ("aux", aux)):
        assert t is None or (t.guards_intact() and (o[k] is None or torch.equal(t.body(), o[k]))), (case.name, k, "an input was written")
    return {k: (t.body() if t is not None else None) for k, t in outs.items()}, (gc.variant_used, gc.bn_used)


def _note(mode, what, ratio):
    _WORST[(mode, what)] = max(_WORST.get((mode, what), 0.0), ratio)


def _written_and_finite(case, d, written):
    assert bool(torch.isfinite(d[written]).all()), (case.name, "an element the reference defines is not finite")
    assert bool(torch.isnan(d[~written]).all()), (case.name, "a row of another phase / past M was written")


def _held(case, what, d, r, bound, mask=None):
    """|d - r| <= bound where mask; prints and notes the worst error / bound."""
    err = (d.to(torch.float64) - r).abs()
    if mask is not None:
        err, bound = err[mask], bound[mask]
    ratio = float((err / bound.clamp(min=1e-300)).max()) if err.numel() else 0.0
    print(f"{case.name} [{what}] worst error / bound {ratio:.4f}, max error {float(err.max()) if err.numel() else 0.0:.3e}, max bound {float(bound.max()) if err.numel() else 0.0:.3e}")
    _note(case.mode, what, ratio)
    assert bool((err <= bound).all()), (case.name, what, ratio)


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print()
    for (mode, what), v in sorted(_WORST.items()):
        print(f"row GEMM mode {mode} [{what}]: worst " + (f"device error {v:.4f} u |x|" if what.startswith("activation") else f"error / bound {v:.4f}"))


@pytest.mark.parametrize("case", R.CASES, ids=lambda c: c.name)
def test_case(case):
    n_cu = _n_cu()
    g = R.geometry(case, n_cu)
    # (a) exact operands
    o = R.operands(case, "exact", n_cu)
    ref = R.reference(case, o, n_cu)
    assert float(ref["S"].max()) < 2.0 ** 24, (case.name, "the exact family needs max S < 2^24")
    out, (variant, bn) = _launch(case, o, n_cu)
    assert bn == g["bn"] and variant == g["variant"], (case.name, "the library chose", variant, bn, "the restated rules", g["variant"], g["bn"])
    w = ref["written"]
    _written_and_finite(case, out["dst"], w)
    if case.linear:
        assert torch.equal(out["dst"][w].to(torch.float64), ref["dst"][w]), (case.name, "exact operands, linear epilogue: not equal", float((out["dst"][w] - ref["dst"][w]).abs().max()))
    if case.dst_pre:
        _written_and_finite(case, out["dst_pre"], w)
        assert torch.equal(out["dst_pre"][w].to(torch.float64), ref["dst_pre"][w].to(torch.float32).to(torch.float64)), (case.name, "exact operands: dst_pre not equal")
    # (b) float operands
    o = R.operands(case, "float", n_cu)
    ref = R.reference(case, o, n_cu)
    out, chosen = _launch(case, o, n_cu)
    assert chosen == (variant, bn)
    _written_and_finite(case, out["dst"], w)
    if not case.linear:  # the device's own pre-activation: the same launch without the activation (and so without the training / sum-of-squares epilogue around it)
        plain = R.replace(case, act=0, dst_pre=False, sq_hw=0)
        po = dict(o, aux=None)
        x = _launch(plain, po, n_cu)[0]["dst"].to(torch.float64)
        pref = R.reference(plain, po, n_cu)
        _held(case, "pre-activation", x, pref["dst"], pref["bound"], w.unsqueeze(1).expand_as(x))
        if not case.scale or case.affine_first:
            if not case.residual:  # the activation alone, on the device's argument: no other rounding between
                name, f = {2: ("gelu", R.gelu64(x)), 4: ("silu", R.silu64(x)), 3: ("gelu_grad", None)}[case.act]
                if case.act == 3:
                    f = x * R.gelu_grad64(o["aux"].to(torch.float64))
                live = w.unsqueeze(1).expand_as(x) & (x != 0)
                c_f = float(((out["dst"].to(torch.float64) - f).abs()[live] / (R.U * x.abs()[live])).max())
                print(f"{case.name} [{name}] device activation error <= {c_f:.3f} u |x|")
                _note(case.mode, "activation " + name, c_f)
                assert R.ACT_BAR[name] is not None and c_f <= R.ACT_BAR[name], (case.name, name, c_f, R.ACT_BAR[name])
    assert ref["bound"] is not None, (case.name, "the activation bars of tests/_row_gemm.py are not measured yet")
    _held(case, "dst", out["dst"], ref["dst"], ref["bound"], w.unsqueeze(1).expand_as(ref["dst"]))
    if case.dst_pre:
        _written_and_finite(case, out["dst_pre"], w)
        if case.act == 3:
            assert torch.equal(out["dst_pre"][w], o["aux"][w]), (case.name, "act 3: dst_pre is aux")
        else:
            _held(case, "dst_pre", out["dst_pre"], ref["dst_pre"], ref["dst_pre_bound"], w.unsqueeze(1).expand_as(ref["dst"]))
    if case.sq_hw:
        sq = out["sumsq"].reshape(ref["sumsq"].shape)
        defined = ~torch.isnan(ref["sumsq"])
        assert bool(torch.isfinite(sq[defined]).all()) and bool(torch.isnan(sq[~defined]).all()), (case.name, "sums of squares: places written / left")
        _held(case, "sumsq", sq, ref["sumsq"], ref["sumsq_bound"], defined)


def test_late_split_does_not_change_a_bit():
    """The same multi-tile persistent case under late_split 0, 1, 2: which waves issue their DMA a step late does not enter the accumulation order."""
    n_cu = _n_cu()
    base = R.BY_NAME[R.LATE_SPLIT_CASE]
    o = R.operands(base, "float", n_cu)
    outs = [_launch(R.with_late_split(base, ls), o, n_cu)[0]["dst"] for ls in (0, 1, 2)]
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])


def test_launch_checks_come_back_as_error_codes():
    n_cu = _n_cu()
    bad = R.replace(R.BY_NAME["m_v0_256"], variant=1)  # the 256x96 variant on a pack with N tile 128
    with pytest.raises(L.PosehipError):
        _launch(bad, R.operands(bad, "exact", n_cu), n_cu)


def test_the_table_reaches_every_variant_mode_and_epilogue():
    """Every (variant, kernel template) pair launch_gemm_variant can dispatch (twice: one case of a pair cannot leave unnoticed), every mode, every epilogue form, per N
    tile a full and a partial last tile; the persistent cases do walk past their first tile on THIS device, under both branches of the XCD dealing; the ring phase
    (stages % 3) takes all three values there."""
    assert R.missing_coverage(R.CASES) == []
    n_cu = _n_cu()
    multi = [R.geometry(c, n_cu) for c in R.CASES if "persist" in c.tags]
    assert all(g["mtiles"] * g["ntc"] > n_cu for g in multi)
    assert {g["mtiles"] % 8 == 0 for g in multi} == {True, False}
    assert {max(g["nstages"], 2) % 3 for g in multi} == {0, 1, 2} and any(g["nstages"] == 1 for g in multi)
    assert any(g["ntc"] >= 3 and g["mtiles"] > n_cu for g in multi) and any(g["ntc"] == 1 and g["mtiles"] > 2 * n_cu for g in multi)
