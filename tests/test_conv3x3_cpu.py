"""The float64 reference of the exact-fp32 3x3 conv tests (tests/_conv3x3.py) held to independent formulations, the conditions its case table rests on, and every case's
route on a 256-CU chip (ph_debug_conv3x3_route: a case that drifts to another kernel fails here, without a GPU).  No GPU.

CONV3X3_RECORD=1 rewrites the MEASURED block of tests/_conv3x3.py (e32 per float case of a Winograd kernel, from the reference's own float32 evaluation)."""
import ctypes as C
import os
import re

import pytest
import torch
import torch.nn.functional as F

from sleap_nn_amd import _lib as L
from tests import _conv3x3 as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLOAT_REFS = {}  # name -> (operands, reference): computed once, shared, never modified


def _float_ref(c):
    if c.name not in FLOAT_REFS:
        o = R.operands(c, "float")
        FLOAT_REFS[c.name] = (o, R.reference(c, o))
    return FLOAT_REFS[c.name]


SMALL = [c for c in R.CASES if "rounds" not in c.tags]


# ---- the entry

def test_run_entry_is_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "posehip.h")).read()
    assert "int ph_debug_conv3x3_run(ph_conv_run_case* c);" in header and int(re.search(r"^#define\s+PH_VERSION\s+(\d+)", header, re.M).group(1)) >= 131
    fields = re.search(r"typedef struct ph_conv_run_case \{(.*?)\} ph_conv_run_case;", header, re.S).group(1)
    names = [n.strip(" *") for decl in fields.split(";") if decl.strip() for n in decl.split(",")]
    names = [n.split()[-1].strip("*") for n in names]
    assert names == [n for n, _ in L.ConvRunCase._fields_]
    assert L.lib().ph_conv_run_case_size() == C.sizeof(L.ConvRunCase)


# ---- the reference against independent formulations

def _bilinear_x2(x):
    """Hand-written bilinear x2, align_corners = False: output i reads source (i + 0.5) / 2 - 0.5, clamped at 0 from below, its upper neighbour clamped at the last index."""
    def axis(t, dim):
        n = t.shape[dim]
        out = []
        for i in range(2 * n):
            s = max((i + 0.5) / 2.0 - 0.5, 0.0)
            i0 = int(s)
            i1, f = min(i0 + 1, n - 1), s - int(s)
            out.append(t.select(dim, i0) * (1.0 - f) + t.select(dim, i1) * f)
        return torch.stack(out, dim)
    return axis(axis(x, 2), 3)


def _conv_by_taps(x, w):
    """Nine shifted matmuls over a zero-padded copy."""
    B, cin, H, W = x.shape
    xp = torch.zeros(B, cin, H + 2, W + 2, dtype=x.dtype)
    xp[:, :, 1 : H + 1, 1 : W + 1] = x
    y = torch.zeros(B, w.shape[0], H, W, dtype=x.dtype)
    for ky in range(3):
        for kx in range(3):
            y += torch.einsum("bchw,oc->bohw", xp[:, :, ky : ky + H, kx : kx + W], w[:, :, ky, kx])
    return y


def _pool_by_loop(y):
    """(B, H, W, c) -> (B, ceil(H/2), ceil(W/2), c), each window over the pixels that exist."""
    B, H, W, c = y.shape
    out = torch.empty(B, (H + 1) // 2, (W + 1) // 2, c, dtype=y.dtype)
    for py in range((H + 1) // 2):
        for px in range((W + 1) // 2):
            out[:, py, px] = y[:, 2 * py : min(2 * py + 2, H), 2 * px : min(2 * px + 2, W)].reshape(B, -1, c).max(1).values
    return out


def test_reference_equals_taps_fold_and_pool_written_out():
    seen = set()
    for c in SMALL:
        g = R.geometry(c)
        o, ref = _float_ref(c)
        x = R._nchw64(o["src0"], c.cin0)
        if c.cin1:
            s1 = R._nchw64(o["src1"], c.cin1)
            x = torch.cat([x, _bilinear_x2(s1) if c.lowres else s1], 1)
        assert x.shape[2:] == (g["H"], g["W"]), c.name
        y = _conv_by_taps(x, o["weight"].to(torch.float64)) + o["bias"].to(torch.float64).view(1, -1, 1, 1)
        assert torch.allclose(ref["conv"], y, rtol=0, atol=1e-12), c.name
        y = R._padc(y, g["coutp"]).permute(0, 2, 3, 1)
        if c.relu:
            y = y.clamp(min=0)
        if c.accumulate:
            y = y + o["old"].to(torch.float64)
        if c.mask:
            y = y * (o["mask"] > 0)
        assert torch.allclose(ref["dst"], y, rtol=0, atol=1e-12), c.name
        pad = ref["dst"][..., c.cout :]
        want = o["old"][..., c.cout :].to(torch.float64) if c.accumulate else torch.zeros_like(pad)
        assert torch.equal(pad, want * (o["mask"][..., c.cout :] > 0) if c.mask else want), (c.name, "pad channels")
        if c.pool:
            assert ref["pool"].shape[1:3] == (g["Hp"], g["Wp"]) and torch.allclose(ref["pool"], _pool_by_loop(y), rtol=0, atol=1e-12), c.name
        if c.head:
            pre = torch.einsum("oc,bhwc->bohw", o["head_w"].to(torch.float64), y[..., : c.cout]) + o["head_b"].to(torch.float64).view(1, -1, 1, 1)
            assert torch.allclose(ref["head_pre"], pre, rtol=0, atol=1e-12) and ref["head"].shape == (g["B"], c.head, g["H"], g["W"]), c.name
            assert torch.allclose(ref["head"], 1.0 / (1.0 + torch.exp(-pre)) if c.sigmoid else pre, rtol=0, atol=1e-15), c.name
        seen |= {k for k in ("lowres", "pool", "head", "mask", "accumulate") if getattr(c, k)}
    assert seen == {"lowres", "pool", "head", "mask", "accumulate"}


def test_fp32_winograd_evaluations_stay_within_their_rigorous_bound():
    """F(2,3), F(2x2,3x3) and F(4x4,3x3) with the textbook matrices: in float64 they are the conv; in float32 they stay within gamma_n x the magnitude sum through the
    absolute-value transforms, and that bound is far above what they actually err by (it is the outer limit, not the bar)."""
    seen = set()
    for c in SMALL:
        if c.direct:
            continue
        o, ref = _float_ref(c)
        m, two_d = R.WINO_M[c.kernel]
        w64 = R.winograd(R.sources(c, o), o["weight"].to(torch.float64), m, two_d) + o["bias"].to(torch.float64).view(1, -1, 1, 1)
        assert torch.allclose(w64, ref["conv"], rtol=0, atol=1e-11), c.name
        rig, mag = R.rigorous_bound(c, o)
        f32 = R.fp32_evaluation(c, o)["dst"].to(torch.float64)
        assert bool(((f32 - ref["dst"]).abs() <= rig).all()), c.name
        assert bool((mag + 1e-12 >= ref["S"]).all()), (c.name, "the transforms' magnitude sum is no smaller than the direct one")
        seen.add((m, two_d))
    assert seen == {(2, False), (2, True), (4, True)}


def test_exact_family_is_exact():
    """The magnitude sum -- through the transforms where the kernel has them -- stays below 2^24 for every exact case, and the reference's values are integers."""
    for c in R.CASES:
        if "rounds" in c.tags and c.name.count("rounds2"):
            continue  # (the same operand ranges and channel counts as its rounds1 twin)
        o = R.operands(c, "exact")
        ref = R.reference(c, o)
        top = float(ref["S"].max())
        if not c.direct:
            top = max(top, float(R.rigorous_bound(c, o)[1].max()))
        if c.head:
            top = max(top, float(ref["S_head"].max()))
        assert top < 2.0 ** 24, (c.name, top)
        assert bool((ref["dst"] == ref["dst"].round()).all()), c.name
        if c.head:
            assert bool((ref["head_pre"] == ref["head_pre"].round()).all()), c.name
        if c.kernel in (R.K_WINO1D, R.K_W16, R.K_WINO2D, R.K_SMALLMAP):  # G only halves: the transformed weights of multiples of 4 are integers
            assert bool((o["weight"] % 4 == 0).all()), c.name
        if c.lowres:
            assert bool((R.sources(c, o) == R.sources(c, o).round()).all()), (c.name, "the folded source holds integers")


# ---- sensitivity: on the reference alone, each mutation breaks the case's bar somewhere

def _mutations(c, g, o, ref):
    """name -> (tensor name, mutated tensor) for every mutation that applies to the case."""
    x = R.sources(c, o)
    w, b = o["weight"].to(torch.float64), o["bias"].to(torch.float64)
    B, H, W = g["B"], g["H"], g["W"]
    th, tw = R.TILE[c.kernel]
    out = {}

    def with_conv(conv):
        return R.epilogue(c, g, o, conv)

    base = ref["conv"]
    # one tap dropped at one border pixel (the last image's last row)
    if W >= 2:
        m = base.clone()
        m[B - 1, :, H - 1, W - 1] -= w[:, :, 1, 0] @ x[B - 1, :, H - 1, W - 2]
        out["tap dropped at a border pixel"] = with_conv(m)
    # one tile column shifted by a pixel
    if W >= 2:
        m = base.clone()
        x0 = tw - 1 if W > tw else 0
        m[:, :, :, x0] = base[:, :, :, x0 + 1] if x0 + 1 < W else base[:, :, :, x0 - 1]
        out["tile column shifted"] = with_conv(m)
    # two output channels swapped across the N-half boundary (32 | 16 | the middle)
    if c.cout >= 2:
        h = 32 if c.cout > 32 else (16 if c.cout > 16 else c.cout // 2)
        m = base.clone()
        m[:, h - 1], m[:, h] = base[:, h], base[:, h - 1]
        out["channels swapped"] = with_conv(m)
    # the last K chunk skipped
    k0 = (g["K"] - 1) // 16 * 16 if not c.cin1 else c.cin0 + (c.cin1 - 1) // 16 * 16
    out["last K chunk skipped"] = with_conv(base - F.conv2d(x[:, k0:], w[:, k0:], padding=1))
    # zero padding replaced by clamping at the top border
    m = base.clone()
    m[:, :, 0] += F.conv1d(x[:, :, 0], w[:, :, 0], padding=1)  # row -1 reads row 0: the ky = 0 taps over row 0
    out["clamped at the top border"] = with_conv(m)
    # pool taken with floor instead of ceil size: the last pooled row / column is never written
    if c.pool and (H & 1 or W & 1):
        p = dict(ref)
        pool = ref["pool"].clone()
        if H & 1:
            pool[:, -1] = R.NAN
        if W & 1:
            pool[:, :, -1] = R.NAN
        p["pool"] = pool
        out["pool of floor size"] = p
    return out


def _breaks(c, o, what, mut, ref, bar):
    def over(d, r, b):
        e = (d - r).abs()
        return bool((torch.isnan(e) | (e > b)).any())
    if what == "pool of floor size":
        return over(mut["pool"], ref["pool"], F.max_pool2d(bar.permute(0, 3, 1, 2), 2, 2, ceil_mode=True).permute(0, 2, 3, 1))
    hit = (not c.skip_dst) and over(mut["dst"], ref["dst"], bar)
    if c.pool:
        hit = hit or over(mut["pool"], ref["pool"], F.max_pool2d(bar.permute(0, 3, 1, 2), 2, 2, ceil_mode=True).permute(0, 2, 3, 1))
    if c.head:
        hit = hit or over(mut["head_pre"], ref["head_pre"], R.head_bar(c, o, ref, bar))
    return hit


@pytest.mark.parametrize("case", SMALL, ids=lambda c: c.name)
def test_mutations_of_the_reference_break_the_bar(case):
    g = R.geometry(case)
    o, ref = _float_ref(case)
    bar = R.dst_bar(case, o, ref)
    muts = _mutations(case, g, o, ref)
    assert len(muts) >= (3 if g["W"] < 2 else 5), case.name
    for what, mut in muts.items():
        assert _breaks(case, o, what, mut, ref, bar), (case.name, what, "does not break the bar")
    if case.pool:
        assert (g["H"] & 1 or g["W"] & 1) == ("pool of floor size" in muts)


def test_every_pool_kernel_has_an_odd_pool_case():
    for k in range(8):
        if k not in (R.K_C16, R.K_WINO4):  # (conv3x3_c16 has no fused pool; F(4x4,3x3) takes H and W in multiples of 4)
            assert any(c.kernel == k and c.pool and (R.geometry(c)["H"] & 1 or R.geometry(c)["W"] & 1) for c in R.CASES), R.KERNEL_NAMES[k]


# ---- the table

def _route(c, n_cu=R.CHIP_CUS):
    g = R.geometry(c, n_cu)
    rc = L.ConvRouteCase(c0p=g["c0p"], c1p=g["c1p"], coutp=g["coutp"], bn=g["bn"], B=g["B"], H=g["H"], W=g["W"], forms=g["forms"], flags=g["flags"], head_cout=c.head,
                         head_wcp=g["coutp"] if c.head else 0, ptr_salt=0, split_scratch_bytes=g["scratch_bytes"], **g["options"])
    out = L.ConvRouteOut()
    L.check(L.lib().ph_debug_conv3x3_route(C.byref(rc), n_cu, C.byref(out)))
    return out


@pytest.mark.parametrize("case", R.CASES, ids=lambda c: c.name)
def test_case_routes_to_its_kernel(case):
    out = _route(case)
    assert (out.kernel, out.ksplit, out.props) == (case.kernel, case.ksplit, R.expected_props(case)), (
        case.name, "routed to", R.KERNEL_NAMES[out.kernel], out.ksplit, out.props, "the case is there for", R.KERNEL_NAMES[case.kernel], case.ksplit, R.expected_props(case))
    if case.scratch == "short":
        assert R.geometry(case)["scratch_bytes"] == R._shape_ksplit(case, R.geometry(case)["c0p"] + R.geometry(case)["c1p"]) * R.geometry(case)["plane"] - 1


def test_the_table_is_complete_and_notices_a_missing_case():
    assert R.missing_coverage(R.CASES) == []
    by_pair = {}
    for c in R.CASES:
        if "pair" in c.tags:
            by_pair.setdefault((c.kernel, R.instantiation(c)), []).append(c.name)
    assert sorted(by_pair) == sorted(R.PAIRS)
    for pair, names in by_pair.items():  # with exactly two cases to a pair, deleting either one must show; with more, deleting down to one must
        gone = [c for c in R.CASES if c.name not in names[: len(names) - 1]]
        assert ("pair",) + pair in R.missing_coverage(gone), pair
    for n_cu in (256, 304, 64):  # the cases that outrun the persistent grid do so on any chip, and the small-map kernel's two-block forms are reached
        assert R.missing_coverage(R.CASES, n_cu) == [], n_cu
        for c in R.CASES:
            if "rounds" in c.tags and dict(c.opts).get("persist", 1):
                grid = n_cu * (4 if c.kernel == R.K_C16 else 1)
                rounds = int(c.name.split("rounds")[1][0])
                assert rounds * grid < R.geometry(c, n_cu)["units"] <= rounds * grid + grid // 2, (c.name, n_cu)


def test_channel_and_map_edges_are_in_the_table():
    for k in (R.K_REGSTAGED, R.K_DMA9, R.K_WINO1D):
        assert {R.geometry(c)["coutp"] for c in R.CASES if c.kernel == k} >= {16, 32, 48, 64, 96, 128}, R.KERNEL_NAMES[k]
    assert {R.geometry(c)["coutp"] for c in R.CASES if c.kernel == R.K_WINO2D} >= {32, 64, 96, 128}
    assert {R.geometry(c)["coutp"] for c in R.CASES if c.kernel == R.K_WINO4} >= {32, 64, 96, 128}
    assert {R.geometry(c)["coutp"] for c in R.CASES if c.kernel == R.K_SMALLMAP} >= {16, 32, 48, 64, 96, 128}
    two = {(R.geometry(c)["c0p"], R.geometry(c)["c1p"], R.geometry(c)["coutp"]) for c in R.CASES if c.kernel == R.K_W16 and c.cin1}
    assert two == {(a, b, n) for a in (16, 32, 48) for b in (16, 32, 48) for n in (16, 32) if R.w16_shape_ok(a, b, n)}
    for k in range(8):
        th, tw = R.TILE[k]
        step = 4 if k == R.K_WINO4 else 1
        maps = {(R.geometry(c)["H"], R.geometry(c)["W"]) for c in R.CASES if c.kernel == k}
        assert maps >= {(th - step, tw - step), (th, tw), (th + step, tw + step)}, R.KERNEL_NAMES[k]
        assert any(c.cout % 16 for c in R.CASES if c.kernel == k) and any((c.cin0 % 16 or c.cin1 % 16) for c in R.CASES if c.kernel == k), R.KERNEL_NAMES[k]
    low = {(R.geometry(c)["H"], R.geometry(c)["W"]) for c in R.CASES if c.lowres}
    assert {(2, 2), (4, 4)} <= low


# ---- the recorded e32

def test_measured_e32_is_the_references_own():
    """Every float case of a Winograd kernel has its e32 in MEASURED, and it is what the reference's float32 evaluation gives here (to a factor: another BLAS sums in another
    order).  CONV3X3_RECORD=1 rewrites the block."""
    now = {}
    for c in R.CASES:
        if not c.direct:
            o, ref = (R.operands(c, "float"), None) if "rounds" in c.tags else _float_ref(c)
            ref = ref or R.reference(c, o)
            now[c.name] = R.e32_of(c, o, ref)
    if os.environ.get("CONV3X3_RECORD") == "1":
        path = os.path.join(ROOT, "tests", "_conv3x3.py")
        src = open(path).read()
        block = "# MEASURED-BEGIN\nMEASURED = {\n" + "".join(f'    "{k}": {v:.4e},\n' for k, v in now.items()) + "}\n# MEASURED-END"
        open(path, "w").write(re.sub(r"# MEASURED-BEGIN.*# MEASURED-END", lambda m: block, src, flags=re.S))
        return
    assert sorted(R.MEASURED) == sorted(now)
    for k, v in now.items():
        assert v > 0 and 0.5 <= R.MEASURED[k] / v <= 2.0, (k, R.MEASURED[k], v)
