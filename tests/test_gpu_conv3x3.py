"""The eight exact-fp32 3x3 conv kernels behind conv3x3_route ("Held to float64 at the tile edges") called one launch at a time through
ph_debug_conv3x3_run on tensors the test owns, against the float64 reference of tests/_conv3x3.py, over its case table.  Per case:

(a) exact operands (small integers): the direct kernels and the F(2,3) / F(2x2,3x3) kernels must EQUAL the reference -- dst, the fused pool and the fused head's
    pre-activation; F(4x4,3x3) is held to its rigorous bound there (tests/_conv3x3.py says why);
(b) float operands: per element within the case's bar (direct kernels: gamma_n S; Winograd kernels: 4 e32, never above the rigorous bound);
(c) every tensor lies between NaN guard pixels in a NaN-filled buffer, the sources too (a tap read outside the first or last image shows in the output); inputs come back
    bit-identical; under skip_dst, dst is still all NaN; under split K the scratch planes beyond ksplit are untouched; everything the reference defines is finite;
(d) the kernel, the K slices and the properties the entry reports are the case's; the split-K counters the entry owns are back to zero.

One process, no subprocesses."""
import ctypes as C

import pytest
import torch

from sleap_nn_amd import _lib as L
from tests import _conv3x3 as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_WORST = {}  # (kernel, what) -> worst error / bar over the cases run so far


def _n_cu():
    return torch.cuda.get_device_properties(0).multi_processor_count


class _Guarded:
    """An NHWC (or NCHW) tensor between NaN guard pixels on either side, on the device; NaN-filled unless `fill` is given."""

    def __init__(self, shape, guard, fill=None):
        self.shape = tuple(shape)
        self.n = 1
        for s in self.shape:
            self.n *= s
        self.g = guard * self.shape[-1]
        self.buf = torch.full((self.n + 2 * self.g,), R.NAN, dtype=torch.float32, device=DEV)
        self.fill = fill
        if fill is not None:
            self.buf[self.g : self.g + self.n] = fill.reshape(-1).to(DEV)

    @property
    def ptr(self):
        return self.buf.data_ptr() + self.g * 4

    def guards_intact(self):
        return bool(torch.isnan(self.buf[: self.g]).all()) and bool(torch.isnan(self.buf[self.g + self.n :]).all())

    def body(self):
        return self.buf[self.g : self.g + self.n].cpu().reshape(self.shape)


def _launch(case, o, n_cu, sigmoid=None):
    """One ph_debug_conv3x3_run -> ({"dst", "pool", "head", "scratch": CPU tensors or None}, the entry's report)."""
    g = R.geometry(case, n_cu)
    gp = R.guard_pixels(g["W"])
    B, H, W = g["B"], g["H"], g["W"]
    src0 = _Guarded((B, H, W, g["c0p"]), gp, o["src0"])
    src1 = _Guarded((B, g["H1"], g["W1"], g["c1p"]), gp, o["src1"]) if case.cin1 else None
    mask = _Guarded((B, H, W, g["coutp"]), gp, o["mask"]) if case.mask else None
    outs = {"dst": _Guarded((B, H, W, g["coutp"]), gp, o["old"] if case.accumulate else None)}
    outs["pool"] = _Guarded((B, g["Hp"], g["Wp"], g["coutp"]), gp) if case.pool else None
    outs["head"] = _Guarded((B, case.head, H, W), gp) if case.head else None
    outs["scratch"] = _Guarded((g["scratch_planes"], B, H, W, g["coutp"]), gp) if case.scratch else None
    host = {k: (o[k].contiguous() if o[k] is not None else None) for k in ("weight", "bias", "head_w", "head_b")}
    rc = L.ConvRunCase(cin0=case.cin0, cin1=case.cin1, cout=case.cout, bn=g["bn"], B=B, H=H, W=W, forms=g["forms"], flags=g["flags"], head_cout=case.head,
                       relu=case.relu, splitk_finish=case.splitk_finish, head_sigmoid=int(case.sigmoid if sigmoid is None else sigmoid), kernel=-9, kv=-9, ksplit=-9, props=-9,
                       n_cu=-9, counters_zero=-9, split_scratch_bytes=g["scratch_bytes"], src0=src0.ptr, src1=src1.ptr if src1 else None, dst=outs["dst"].ptr,
                       dst_pool=outs["pool"].ptr if outs["pool"] else None, relu_mask_src=mask.ptr if mask else None, head_dst=outs["head"].ptr if outs["head"] else None,
                       split_scratch=outs["scratch"].ptr if outs["scratch"] else None, weight=host["weight"].data_ptr(), bias=host["bias"].data_ptr(),
                       head_w=host["head_w"].data_ptr() if case.head else None, head_b=host["head_b"].data_ptr() if case.head else None, **g["options"])
    torch.cuda.synchronize()
    L.check(L.lib().ph_debug_conv3x3_run(C.byref(rc)))
    for k, t in outs.items():
        assert t is None or t.guards_intact(), (case.name, k, "a guard pixel was written")
    for k, t in (("src0", src0), ("src1", src1), ("mask", mask)):
        assert t is None or (t.guards_intact() and torch.equal(t.body(), o[k])), (case.name, k, "an input was written")
    return {k: (t.body() if t is not None else None) for k, t in outs.items()}, rc


def _reported(case, rc, n_cu):
    assert rc.n_cu == n_cu, (case.name, "the entry asked the route with", rc.n_cu, "CUs, the device has", n_cu)
    assert (rc.kernel, rc.ksplit, rc.props) == (case.kernel, case.ksplit, R.expected_props(case)), (
        case.name, "routed to", R.KERNEL_NAMES[rc.kernel], rc.ksplit, rc.props, "the case is there for", R.KERNEL_NAMES[case.kernel], case.ksplit, R.expected_props(case))
    assert rc.counters_zero == 1, (case.name, "the split-K counters are not back to zero")


def _stray(case, out, rc):
    """What the launch must leave alone, and that all it defines is finite."""
    if case.skip_dst:
        assert bool(torch.isnan(out["dst"]).all()), (case.name, "skip_dst: dst was written")
    else:
        assert bool(torch.isfinite(out["dst"]).all()), (case.name, "dst: an element is not finite (an unwritten element, or a tap read outside its image)")
    for k in ("pool", "head"):
        assert out[k] is None or bool(torch.isfinite(out[k]).all()), (case.name, k, "an element is not finite")
    if out["scratch"] is not None:
        used = rc.ksplit if rc.ksplit > 1 else 0
        assert bool(torch.isnan(out["scratch"][used:]).all()), (case.name, "split scratch beyond", used, "planes was written")
        assert bool(torch.isfinite(out["scratch"][:used]).all()), (case.name, "a split-K plane holds a non-finite partial sum")


def _held(case, what, d, r, bar):
    """|d - r| <= bar per element; prints and notes the worst error / bar."""
    err = (d.to(torch.float64) - r).abs()
    bar = bar if torch.is_tensor(bar) else torch.full_like(err, bar)
    ratio = float((err / bar.clamp(min=1e-300)).max())
    print(f"{case.name} [{what}] worst error / bar {ratio:.4f}, max error {float(err.max()):.3e}, max bar {float(bar.max()):.3e}")
    _WORST[(case.kernel, what)] = max(_WORST.get((case.kernel, what), 0.0), ratio)
    assert bool((err <= bar).all()), (case.name, what, ratio)


def _pool_bar(bar):
    """The bar of a max over a 2 x 2 window: the largest of the window's bars."""
    return torch.nn.functional.max_pool2d(bar.permute(0, 3, 1, 2), 2, 2, ceil_mode=True).permute(0, 2, 3, 1)


def _compare_float(case, o, ref, out, n_cu, e32=None):
    bar = R.dst_bar(case, o, ref, n_cu, e32)
    if not case.skip_dst:
        _held(case, "dst", out["dst"], ref["dst"], bar)
        assert torch.equal(out["dst"][..., case.cout :].to(torch.float64), ref["dst"][..., case.cout :]), (case.name, "pad channels of dst")
    if case.pool:
        _held(case, "pool", out["pool"], ref["pool"], _pool_bar(bar))
    return bar


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print()
    for (kernel, what), v in sorted(_WORST.items()):
        unit = "u" if what == "sigmoid" else ("e32" if what.endswith("/ e32") else "bar")
        print(f"3x3 conv, {R.KERNEL_NAMES[kernel]} [{what}]: worst {v:.4f} {unit}")


@pytest.mark.parametrize("case", R.CASES, ids=lambda c: c.name)
def test_case(case):
    n_cu = _n_cu()
    # (a) exact operands
    o = R.operands(case, "exact", n_cu)
    ref = R.reference(case, o, n_cu)
    out, rc = _launch(case, o, n_cu, sigmoid=False)
    _reported(case, rc, n_cu)
    _stray(case, out, rc)
    if case.kernel == R.K_WINO4:
        rig, mag = R.rigorous_bound(case, o, n_cu)
        assert float(mag.max()) < 2.0 ** 24
        if not case.skip_dst:
            _held(case, "exact operands, dst", out["dst"], ref["dst"], rig)
        if case.pool:
            _held(case, "exact operands, pool", out["pool"], ref["pool"], _pool_bar(rig))
    else:
        if not case.skip_dst:
            assert torch.equal(out["dst"].to(torch.float64), ref["dst"]), (case.name, "exact operands: dst not equal", float((out["dst"] - ref["dst"]).abs().max()))
        if case.pool:
            assert torch.equal(out["pool"].to(torch.float64), ref["pool"]), (case.name, "exact operands: pool not equal", float((out["pool"] - ref["pool"]).abs().max()))
        if case.head:
            assert torch.equal(out["head"].to(torch.float64), ref["head_pre"]), (case.name, "exact operands: head not equal", float((out["head"] - ref["head_pre"]).abs().max()))
    # (b) float operands
    o = R.operands(case, "float", n_cu)
    ref = R.reference(case, o, n_cu)
    out, rc = _launch(case, o, n_cu)
    _reported(case, rc, n_cu)
    _stray(case, out, rc)
    bar = _compare_float(case, o, ref, out, n_cu)
    if not case.direct and not case.skip_dst:
        worst = float((out["dst"].to(torch.float64) - ref["dst"]).abs().max()) / R.case_e32(case, o, ref, n_cu)
        _WORST[(case.kernel, "error / e32")] = max(_WORST.get((case.kernel, "error / e32"), 0.0), worst)
    if case.head:
        pre = out["head"]
        if case.sigmoid:  # the device's own pre-activation: the same launch without the sigmoid
            pre = _launch(case, o, n_cu, sigmoid=False)[0]["head"]
            again = _launch(case, o, n_cu, sigmoid=False)[0]["head"]
            assert torch.equal(pre, again), (case.name, "two launches of one case differ")
            x = pre.to(torch.float64)
            c_s = float(((out["head"].to(torch.float64) - torch.sigmoid(x)).abs() / R.U).max())
            print(f"{case.name} [sigmoid] device sigmoid error <= {c_s:.3f} u")
            _WORST[(case.kernel, "sigmoid")] = max(_WORST.get((case.kernel, "sigmoid"), 0.0), c_s)
            assert R.SIGMOID_BAR is not None and c_s <= R.SIGMOID_BAR, (case.name, "sigmoid", c_s, R.SIGMOID_BAR)
        _held(case, "head pre-activation", pre, ref["head_pre"], R.head_bar(case, o, ref, bar))


def test_sigmoid_pair_has_one_pre_activation():
    """A sigmoid head and the same launch without the sigmoid differ in nothing but the head's last step: dst is bitwise equal, the launch without the sigmoid repeats bit
    for bit, and the sigmoid launch's output is the device sigmoid of exactly that pre-activation (within the device function's own bar, far below what one ulp more or
    less of a pre-activation near zero would move it by)."""
    n_cu = _n_cu()
    for name in ("w16_head16_16_sig1", "wino2d_head32_sig1", "sm_head17_sig1"):
        case = R.BY_NAME[name]
        o = R.operands(case, "float", n_cu)
        with_s, _ = _launch(case, o, n_cu, sigmoid=True)
        without, _ = _launch(case, o, n_cu, sigmoid=False)
        again, _ = _launch(case, o, n_cu, sigmoid=False)
        assert case.skip_dst or torch.equal(with_s["dst"], without["dst"]), name
        assert torch.equal(without["head"], again["head"]), name
        err = (with_s["head"].to(torch.float64) - torch.sigmoid(without["head"].to(torch.float64))).abs()
        assert R.SIGMOID_BAR is not None and float(err.max()) <= R.SIGMOID_BAR * R.U, (name, float(err.max()) / R.U)


def test_split_k_counters_return_to_zero_and_second_stage_forms_agree():
    """The in-kernel second stage (splitk_finish = 1) and the two-launch form sum the same planes in the same fixed order: equal bit for bit; the counters the entry owns are
    zero again after either."""
    n_cu = _n_cu()
    for name in ("wino2d_splitk2_finish1", "wino2d_splitk_pool_finish", "wino2d_splitk_clamped_finish"):
        case = R.BY_NAME[name]
        o = R.operands(case, "float", n_cu)
        a, rc_a = _launch(case, o, n_cu)
        b, rc_b = _launch(R.replace(case, splitk_finish=0), o, n_cu)
        assert rc_a.counters_zero == 1 and rc_b.counters_zero == 1 and rc_a.ksplit == rc_b.ksplit == case.ksplit
        assert torch.equal(a["dst"], b["dst"]) and (a["pool"] is None or torch.equal(a["pool"], b["pool"])), name


def test_same_operands_through_other_kernels():
    """One set of float operands through four kernels, each held to the reference on its own bar."""
    n_cu = _n_cu()
    base = R.BY_NAME[R.CROSS_CHECK[0]]
    o = R.operands(base, "float", n_cu)
    ref = R.reference(base, o, n_cu)
    for kernel in (base.kernel,) + R.CROSS_CHECK[1]:
        case = R.replace(base, kernel=kernel)
        out, rc = _launch(case, o, n_cu)
        assert rc.kernel == kernel, (R.KERNEL_NAMES[kernel], rc.kernel)
        _compare_float(case, o, ref, out, n_cu, e32=None if case.direct else R.e32_of(case, o, ref, n_cu))


def test_a_changed_operand_element_fails_the_comparison():
    """Per kernel, both families: one element of a source changed between the reference and the launch breaks equality / the bar."""
    n_cu = _n_cu()
    for kernel in range(8):
        case = next(c for c in R.CASES if c.kernel == kernel and "pair" in c.tags and not c.skip_dst)
        for family in ("exact", "float"):
            o = R.operands(case, family, n_cu)
            ref = R.reference(case, o, n_cu)
            g = R.geometry(case, n_cu)
            bent = dict(o, src0=o["src0"].clone())
            bent["src0"][g["B"] - 1, g["H"] - 1, g["W"] // 2, 0] += 1.0 if family == "exact" else 0.25
            out, _ = _launch(case, bent, n_cu)
            if family == "exact" and kernel != R.K_WINO4:
                assert not torch.equal(out["dst"].to(torch.float64), ref["dst"]), (case.name, family)
            else:
                bar = R.rigorous_bound(case, o, n_cu)[0] if family == "exact" else R.dst_bar(case, o, ref, n_cu)
                assert bool(((out["dst"].to(torch.float64) - ref["dst"]).abs() > bar).any()), (case.name, family)


def test_launch_checks_come_back_as_error_codes():
    n_cu = _n_cu()
    for name, change in (("dma9_bn64_16x32", dict(mask=True)),     # a ReLU mask inside the LDS-DMA family on a kernel that applies none: launch_conv3x3_routed's own check
                         ("reg_bn32_8x32", dict(mask=True)),       # ... outside the family: the entry's
                         ("dma9_bn64_16x32", dict(head=5)),        # a head on a kernel that carries none
                         ("wino2d_head32_sig0", dict(head=33)),    # more head channels than the wave-split form takes
                         ("reg_bn64_8x32", dict(lowres=True))):    # a half-resolution source on a kernel that does not fold it
        bad = R.replace(R.BY_NAME[name], **change)
        with pytest.raises(L.PosehipError):
            _launch(bad, R.operands(bad, "exact", n_cu), n_cu)


def test_the_table_reaches_every_pair_on_this_device():
    """Every (kernel, instantiation) pair and epilogue form on THIS device's CU count; the persistent cases do walk past one and past two rounds of its grid."""
    n_cu = _n_cu()
    assert R.missing_coverage(R.CASES, n_cu) == []
    for c in R.CASES:
        if "rounds" in c.tags and c.kernel in R.PERSISTENT and dict(c.opts).get("persist", 1):
            grid = n_cu * (4 if c.kernel == R.K_C16 else 1)
            rounds = int(c.name.split("rounds")[1][0])
            units = R.geometry(c, n_cu)["units"]
            assert rounds * grid < units <= rounds * grid + grid // 2, (c.name, units, grid)
