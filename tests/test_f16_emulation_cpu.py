"""tests/_f16_emulation.py is itself pinned, on the CPU: with nothing rounded it is the oracle; a conforming stand-in (the same storage plan in torch fp32) stays inside
its bound on every tensor of every case of tests/_f16_cases.py; and each of six subtly wrong stand-ins is rejected -- three of them while still passing the yardstick
the plain-fp16 UNet pipe had before (5e-3 absolute at the heads against the fp32 oracle)."""
import pytest
import torch

from oracle import cpu_ref as O
from tests import _f16_cases as T
from tests import _f16_emulation as E

OLD_BAR = 5e-3  # tests/test_gpu_f16_pipe.py: FP16_ATOL, the reference's own autocast tolerance


def _head_names(case):
    return [h for h, _ in O.HEAD_ORDER[case.model_type]]


def _checks(case, device, fused_heads=()):
    """Every tensor of a (stand-in) device run against the emulation, teacher-forced from the device's own tensors: {key: (worst |d - r| - e, share of d != r, worst |d - r| / e)}."""
    sd, img = T.inputs(case)
    forced = {k[1]: v for k, v in device.items() if k[0] == "slot"}
    emu = E.Emulation(T.model(case), sd, fused_heads=fused_heads, **T.emulation_kwargs(case))
    em = emu.run(img, forced)
    return {k: E.check(device[k], *em[k]) for k in em}, emu.behind_unstored


@pytest.mark.parametrize("case", T.CASES, ids=lambda c: c.name)
def test_with_nothing_rounded_the_emulation_is_the_oracle(case):
    sd, img = T.inputs(case)
    m = T.model(case)
    collect = {}
    ref = O.model_forward({k: v.double() for k, v in sd.items()}, case.bb, case.heads, case.model_type, img, collect=collect)
    em = E.Emulation(m, sd, rounded=False).run(img)
    for i, name in enumerate(_head_names(case)):
        r, e = em[("head", i)]
        assert float((r - ref[name]).abs().max()) <= 1e-12 and float(e.max()) == 0.0, name
    seen = 0
    for label, slot in m.backbone.labels.items():
        if ("slot", slot) in em and label in collect:
            assert float((em[("slot", slot)][0] - collect[label]).abs().max()) <= 1e-12, label
            seen += 1
    assert seen >= 3


@pytest.mark.parametrize("case", T.CASES, ids=lambda c: c.name)
def test_the_fp32_standin_stays_inside_the_bound(case):
    """The stand-in satisfies |d - r| <= e on every tensor, teacher-forced (each layer against its own inputs) and chained (bounds propagated from the image).  Its share of
    d != r stays under STANDIN_SHARE (a quarter of the cap the device test may fall back on) on every fp16 tensor whose inputs were all stored, and under twice that on a tensor
    behind an intermediate that is never stored (the stem's full-resolution output: a flip in the halo tile moves 9 x 16 sums) -- so 2 s_ref never reaches the cap either."""
    sd, img = T.inputs(case)
    m = T.model(case)
    heads = [i for i, op in enumerate(m.ops) if op.kind == E.L.OP_HEAD]
    for fused in ((), tuple(heads)):  # both forms of the head weights
        dev = E.standin(m, sd, img, fused_heads=fused, **T.emulation_kwargs(case))
        res, behind = _checks(case, dev, fused)
        worst_share, worst_behind = 0.0, 0.0
        for key, (over, share, _ratio) in res.items():
            assert over <= 0.0, (case.name, key, over)
            if key[0] != "head" and key in behind:
                worst_behind = max(worst_behind, share)
            elif key[0] != "head":
                worst_share = max(worst_share, share)
        chained = E.Emulation(m, sd, fused_heads=fused, **T.emulation_kwargs(case)).run(img)
        for key, (r, e) in chained.items():
            assert E.check(dev[key], r, e)[0] <= 0.0, (case.name, "chained", key)
        print(f"{case.name}: stand-in share of d != r (teacher-forced, {'fused' if fused else 'fp32'} head weights): worst stored-input tensor {worst_share:.2e}, worst tensor behind an unstored one {worst_behind:.2e}")
        assert worst_share <= T.STANDIN_SHARE and worst_behind <= 2 * T.STANDIN_SHARE, (case.name, worst_share, worst_behind)


# (mutation, the cases it is applied to): each case has the structure the mutation needs
MUTATION_CASES = {
    "truncate_store": ("persist_cin16_cin48", "rows_a_mt3_mg4"),
    "fp16_chunk_sums": ("persist_cin16_cin48", "rows_a_mt3_mg4"),          # Cin 48, 16 + 48, 64, 64 + 64: two to four 32-channel chunks
    "bias_after_rounding": ("persist_cin16_cin48", "rows_a_mt3_mg4"),
    "bilinear_last_row_tap": ("persist_cin16_cin48", "upsample_fp32math_standalone"),  # both blend arithmetics
    "double_rounded_intermediate": ("persist_cin16_cin48", "block2_gray_dst_full"),    # the stem's halo tile, the first conv of a block
    "right_border_tap_dropped": ("persist_cin16_cin48", "rows_a_mt3_mg4"),
}
OLD_BAR_BLIND = ("truncate_store", "fp16_chunk_sums", "bias_after_rounding")  # the gap: these pass the old yardstick


@pytest.mark.parametrize("mutation", E.MUTATIONS)
def test_a_subtly_wrong_standin_is_rejected(mutation):
    for name in MUTATION_CASES[mutation]:
        case = T.BY_NAME[name]
        sd, img = T.inputs(case)
        m = T.model(case)
        dev = E.standin(m, sd, img, mutation=mutation, **T.emulation_kwargs(case))
        res, _behind = _checks(case, dev)
        rejected = sorted((k for k, v in res.items() if v[0] > 0.0), key=str)
        ref = O.model_forward(sd, case.bb, case.heads, case.model_type, img)
        old = max(float((dev[("head", i)] - ref[n]).abs().max()) for i, n in enumerate(_head_names(case)))
        print(f"{mutation} on {name}: old bar ({OLD_BAR:g} at the heads): {'passes' if old <= OLD_BAR else 'fails'} ({old:.2e}) / new check: "
              f"{'fails' if rejected else 'passes'} ({len(rejected)} of {len(res)} tensors, worst excess {max(v[0] for v in res.values()):.2e})")
        assert rejected, (mutation, name)
        if mutation in OLD_BAR_BLIND:
            assert old <= OLD_BAR, (mutation, name, old)


def test_check_counts_what_it_says():
    r = torch.tensor([1.0, 2.0, 3.0, 4.0], dtype=torch.float64)
    e = torch.tensor([0.0, 0.5, 0.0, 0.25], dtype=torch.float64)
    over, share, ratio = E.check(torch.tensor([1.0, 2.25, 3.0, 4.5]), r, e)
    assert over == 0.25 and share == 0.5 and ratio == 2.0


def test_fl16_is_round_to_nearest_even_with_subnormals():
    x = torch.tensor([1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 2.0 ** -25, 3 * 2.0 ** -25, 65504.0, 0.1], dtype=torch.float64)
    want = torch.tensor([1.0, 1.0 + 2.0 ** -9, 0.0, 2.0 ** -23, 65504.0, float(torch.tensor(0.1).half())], dtype=torch.float64)
    assert torch.equal(E.fl16(x), want) and torch.equal(E.fl16(-x), -want)
    g = torch.Generator().manual_seed(0)
    v = (torch.rand(20000, generator=g, dtype=torch.float32) - 0.5) * 4
    assert torch.equal(E.fl16(v.double()), v.half().double())  # (fp32 -> fp16 is one rounding)


def test_the_library_declares_the_rows_plan_record():
    import os

    from sleap_nn_amd import _lib as L

    assert L.SIGNATURES["ph_model_last_rows_plans"] == L.SIGNATURES["ph_model_last_kernels"]
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "posehip.h")).read()
    assert "int ph_model_last_rows_plans(const ph_model* m, int32_t* quad, int32_t n_ops);" in header and '"conv_f16_rows_pin"' in header
