"""Every kernel of the plain-fp16 UNet pipe (csrc/f16_kernels.hip, csrc/f16_rows_kernels.hip) against the float64 emulation of its storage contract
(tests/_f16_emulation.py), over the table of tests/_f16_cases.py.  Per case:

(a) keep-everything plan (workspace_reuse 0): every tensor is read back and checked against the emulation restarted from the device's own inputs -- |d - r| <= e;
(b) the inference plan with a range per slot (workspace_reuse 2: the routing, fusions and skipped stores of the default plan): the same, teacher-forced across each fused
    form -- the tensors a fusion keeps out of HBM (block2's tile, the folded bilinear, a pool-only or head-only conv output) are not read, the bound propagates through
    them; then the default plan (workspace_reuse 1) must report the same kernels and give the same bits at the heads, which are also held to the bound propagated from
    the image alone (a worst-case bound: beyond three or four stored tensors it says little, the teacher-forced checks carry the weight);
(c) a second forward of every plan is bitwise equal.

The bound has no floor and no slack.  The share of elements with d != r is held to max(floor, 2 s_ref) per case and tensor class (all inputs stored | behind a tensor that
is never stored), s_ref the share of the torch-fp32 stand-in under the same forcing; floors in ``_f16_cases.MEASURED``."""
import pytest
import torch

from sleap_nn_amd import _lib as L
from tests import _f16_cases as T
from tests import _f16_emulation as E

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_SEEN = {}  # case name -> set of forms its forwards reported (filled by test_case, read by the closure test)


def _forward(case, reuse):
    """-> (model, [head tensors by out_index], kernels, rows plans); the forward runs twice and must repeat bit for bit."""
    _sd, img = T.inputs(case)
    m = T.model(case)
    m.set_option("workspace_reuse", reuse)
    for k, v in case.options.items():
        m.set_option(k, v)
    if case.pin:
        r, wt, mg = case.pin
        m.set_option("conv_f16_rows_pin", r | (wt << 8) | (mg << 16))
    m.to(DEV).set_precision("fp16")
    x = img.to(DEV)
    out = [v.cpu().clone() for v in m(x).values()]
    again = [v.cpu() for v in m(x).values()]
    for a, b in zip(out, again):
        assert torch.equal(a, b), (case.name, reuse, "not repeatable")
    return m, out, list(m.last_kernels()), m.last_rows_plans()


def _forms(m, kv, plans):
    """What the library's records say ran: ("kv", code), ("rows", aligned, MT, MG), ("persist", N tile [+ "+head"])."""
    seen = set()
    for i, (op, code, (r, wt, mt, mg)) in enumerate(zip(m.ops, kv, plans)):
        seen.add(("kv", code))
        if code == L.KV_F16_ROWS:
            assert r > 0 and wt > 0 and 3 <= mt <= 9 and mg in (2, 4) and r * wt <= 16 * mt * mg, (i, r, wt, mt, mg)
            seen.add(("rows", wt % 16 == 0, mt, mg))
        else:
            assert (r, wt, mt, mg) == (0, 0, 0, 0), (i, code)
        if code == L.KV_F16:
            cout_padded = (op.cout + 31) // 32 * 32  # (the fp16 format pads channels to 32; the library's N tile is 64 from 64 padded output channels on)
            head = any(h.kind == L.OP_HEAD and h.src0 == op.dst and kv[j] == L.KV_FUSED for j, h in enumerate(m.ops))
            seen.add(("persist", ("64" if cout_padded >= 64 else "32") + ("+head" if head else "")))
    return seen


def _stored_slots(m, kv):
    """Slots the launches of a fused plan stored and somebody reads back from memory: not the first conv's output of a block2 launch, not a bilinear no launch produced,
    not a tensor whose only readers ride in its producer's epilogue (the store may be skipped)."""
    launched = {r[0] for r in m.last_ranges()}  # ops with a launch of their own
    stored = set()
    for i, op in enumerate(m.ops):
        for slot in (op.dst, op.dst2):
            if slot < 0 or op.kind == L.OP_HEAD:
                continue
            if slot == op.dst and (kv[i] == L.KV_F16_BLOCK or (op.kind == L.OP_UPSAMPLE and i not in launched)):
                continue
            # who reads it from memory: any reader but a head in its producer's epilogue (a folded bilinear counts: the conv behind it reads the slot itself)
            if any(slot in (o.src0, o.src1) and not (o.kind == L.OP_HEAD and kv[j] == L.KV_FUSED) for j, o in enumerate(m.ops)):
                stored.add(slot)
    return stored


def _against_emulation(case, m, heads, kv, slots, shapes, label):
    """Reads `slots` back, restarts the emulation from them and checks every read tensor and every head.  -> (worst |d - r| / e, {class: worst share of d != r}, forced)."""
    sd, img = T.inputs(case)
    forced = {s: m.read_slot(s, shapes[s][1], shapes[s][2:]).cpu() for s in sorted(slots)}
    fused = [i for i, (op, code) in enumerate(zip(m.ops, kv)) if op.kind == L.OP_HEAD and code == L.KV_FUSED]
    emu = E.Emulation(m, sd, fused_heads=fused, **T.emulation_kwargs(case))
    em = emu.run(img, forced)
    worst_ratio, shares = 0.0, {"stored": 0.0, "behind": 0.0}
    for key, (r, e) in em.items():
        if key[0] == "slot" and key[1] in forced:
            d = forced[key[1]]
        elif key[0] == "head":
            d = heads[key[1]]
        else:
            continue
        over, share, ratio = E.check(d, r, e)
        print(f"{case.name} [{label}] {key}: |d - r| - e <= {over:.3e}, worst |d - r| / e {ratio:.3f}, share d != r {share:.2e}, max e {float(e.max()):.2e}")
        assert over <= 0.0, (case.name, label, key, over)
        worst_ratio = max(worst_ratio, ratio)
        if key[0] == "slot":
            cls = "behind" if key in emu.behind_unstored else "stored"
            shares[cls] = max(shares[cls], share)
    return worst_ratio, shares, forced, fused


def _standin_shares(case, m, slots, fused):
    """The torch-fp32 stand-in under the same forcing pattern: {class: worst share of d != r}."""
    sd, img = T.inputs(case)
    dev = E.standin(m, sd, img, fused_heads=fused, **T.emulation_kwargs(case))
    emu = E.Emulation(m, sd, fused_heads=fused, **T.emulation_kwargs(case))
    em = emu.run(img, {s: dev[("slot", s)] for s in slots})
    shares = {"stored": 0.0, "behind": 0.0}
    for s in slots:
        over, share, _ = E.check(dev[("slot", s)], *em[("slot", s)])
        assert over <= 0.0
        cls = "behind" if ("slot", s) in emu.behind_unstored else "stored"
        shares[cls] = max(shares[cls], share)
    return shares


@pytest.mark.parametrize("name", [c.name for c in T.CASES])
def test_case(name):
    case = T.BY_NAME[name]
    sd, img = T.inputs(case)
    seen = set()
    # shapes of every tensor, and the bound propagated from the image alone
    m0 = T.model(case)
    chained = E.Emulation(m0, sd, **T.emulation_kwargs(case)).run(img)
    shapes = {k[1]: tuple(v[0].shape) for k, v in chained.items() if k[0] == "slot"}

    # (a) keep-everything plan
    m, heads, kv, plans = _forward(case, 0)
    seen |= _forms(m, kv, plans)
    every = {s for op in m.ops if op.kind != L.OP_HEAD for s in (op.dst, op.dst2) if s >= 0}
    ratio_a, shares_a, _forced, fused_a = _against_emulation(case, m, heads, kv, every, shapes, "keep")
    ref_a = _standin_shares(case, m, every, fused_a)

    # (b) the inference plan, a range per slot: teacher-forced across the fused forms
    m2, heads2, kv2, plans2 = _forward(case, 2)
    seen |= _forms(m2, kv2, plans2)
    stored = _stored_slots(m2, kv2)
    ratio_b, shares_b, _forced2, fused_b = _against_emulation(case, m2, heads2, kv2, stored, shapes, "inference")
    ref_b = _standin_shares(case, m2, stored, fused_b)
    # ... and the default plan: the same kernels, the same bits, inside the bound propagated from the image
    m1, heads1, kv1, plans1 = _forward(case, 1)
    assert kv1 == kv2 and plans1 == plans2, (kv1, kv2, plans1, plans2)
    em1 = E.Emulation(m1, sd, fused_heads=fused_b, **T.emulation_kwargs(case)).run(img)
    for i, (h1, h2) in enumerate(zip(heads1, heads2)):
        assert torch.equal(h1, h2), (name, "head", i, "default plan differs from the range-per-slot plan")
        assert E.check(h1, *em1[("head", i)])[0] <= 0.0, (name, "head", i, "chained")

    _SEEN[name] = seen
    for form in case.must:
        assert tuple(form) in seen, (name, form, sorted(seen, key=str))

    worst_share = max(list(shares_a.values()) + list(shares_b.values()))
    print(f"{name}: MEASURED ({max(ratio_a, ratio_b):.3f}, {worst_share:.3e}); stand-in keep {ref_a}, inference {ref_b}; device keep {shares_a}, inference {shares_b}; floor {case.floor}")
    assert case.floor is not None, f"{name} has no entry in _f16_cases.MEASURED"
    for shares, ref in ((shares_a, ref_a), (shares_b, ref_b)):
        for cls in shares:
            assert shares[cls] <= T.SHARE_CAP, (name, cls, shares[cls])
            assert shares[cls] <= max(case.floor, 2.0 * ref[cls]), (name, cls, shares[cls], ref[cls], case.floor)


def test_the_table_reaches_every_form():
    """The union over the table of what ``last_rows_plans()`` and ``last_kernels()`` report covers every instantiation launch_conv3x3_f16_rows builds, the persistent
    kernel's three plain-fp16 instantiations and every kernel family of the pipe, but for ``UNREACHED``.  A form added later without a case fails here."""
    for c in T.CASES:  # (run alone, this test takes the forwards itself)
        if c.name not in _SEEN:
            seen = set()
            for reuse in (0, 1):
                m, _heads, kv, plans = _forward(c, reuse)
                seen |= _forms(m, kv, plans)
            _SEEN[c.name] = seen
    seen = set().union(*_SEEN.values())
    rows = {f[1:] for f in seen if f[0] == "rows"}
    assert rows == T.ROWS_BUILT, (sorted(T.ROWS_BUILT - rows), sorted(rows - T.ROWS_BUILT))
    assert {f[1] for f in seen if f[0] == "persist"} >= {"64", "32", "64+head"}, seen
    for code in (L.KV_F16, L.KV_F16_ROWS, L.KV_F16_BLOCK, L.KV_STEM, L.KV_FUSED):
        assert ("kv", code) in seen, L.KV_NAMES[code]
    assert set(T.UNREACHED) == {"pool2x2_fmt_kernel"}  # (no record names it: Model._fuse_pools leaves a UNet's inference program without an OP_POOL)
    for c in T.CASES:
        assert not any(op.kind == L.OP_POOL for op in T.model(c).ops), c.name


def test_the_record_and_the_pin_leave_a_default_forward_alone():
    """cfg5's network at 192 x 192, default options: the pin at 0 and the record change neither the kernels nor the plans; a pinned handle runs the pinned tile where it fits
    and what the search gives elsewhere, and going back to 0 gives the default's bits again."""
    from oracle import cpu_ref as O

    bb = T._unet(16, 2, 32, output_stride=4)
    heads, mt = T._multiclass(5, 4)
    sd = O.init_state(bb, heads, mt, seed=208, head_scale=1.0)
    img = torch.randint(0, 256, (2, 1, 192, 192), dtype=torch.uint8, generator=torch.Generator().manual_seed(192))
    from sleap_nn_amd.architectures.model import Model

    m = Model("unet", bb, heads, mt)
    m.load_state_dict(sd)
    m.to(DEV).set_precision("fp16")
    x = img.to(DEV)
    base = [v.cpu().clone() for v in m(x).values()]
    kv, plans = list(m.last_kernels()), m.last_rows_plans()
    assert m.get_option("conv_f16_rows_pin") == 0.0
    assert all((p != (0, 0, 0, 0)) == (c == L.KV_F16_ROWS) for p, c in zip(plans, kv)) and L.KV_F16_ROWS in kv
    m.set_option("conv_f16_rows", 2)
    free = [v.cpu().clone() for v in m(x).values()]
    fplans = m.last_rows_plans()
    m.set_option("conv_f16_rows_pin", 4 | (48 << 8) | (4 << 16))  # 4 x 48 pixels: maps from 48 pixels wide on
    pinned = [v.cpu().clone() for v in m(x).values()]
    pplans = m.last_rows_plans()
    assert any(p == (4, 48, 3, 4) for p in pplans)
    assert all(p == (4, 48, 3, 4) or p == q for p, q in zip(pplans, fplans)), (pplans, fplans)  # the pinned tile where it fits, the search's choice elsewhere
    m.set_option("conv_f16_rows_pin", 0)
    m.set_option("conv_f16_rows", 1)
    back = [v.cpu() for v in m(x).values()]
    assert list(m.last_kernels()) == kv and m.last_rows_plans() == plans
    for a, b, f, p in zip(base, back, free, pinned):
        assert torch.equal(a, b)
        assert float((f - p).abs().max()) <= 2e-3 * max(1.0, float(a.abs().max()))  # (another tile, the same K order: a few fp32 roundings of sums -- tests/test_gpu_f16_pipe.py's figure between kernels)
