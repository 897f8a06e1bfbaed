"""GPU parity of Swinv2 backbones whose effective windows exceed 8 (the key-tiled kernel window_attn_v2_wide_kernel behind ``allow_swinv2_wide``), inference, exact
fp32: fixtures C (window 16, the 12to16 form) and D (window 12) of tests/_swinv2_wide_cases.py against the reference's own outputs
(tests/golden/pretrained_swinv2_<c|d>*.npz: tools/gen_pretrained_swinv2_wide_golden.py), fixture E (window 24) against tests/swinv2_ref.py in float64.

The bar is the family's: max error <= 1e-4 of max(1, scale) per map.  Measured worst errors are in DESIGN 4.4i."""
import numpy as np
import pytest
import torch

from oracle import cpu_ref as O
from tests import _swinv2_wide_cases as WC
from tests import swinv2_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ATOL = 1e-4
ENC, HEAD = WC.ENC, WC.HEAD


def _err(got, want):
    want = torch.as_tensor(want)
    return (got.double() - want.double()).abs().max().item() / max(1.0, want.abs().max().item())


def _model(name, tmp_path, keep=False):
    m = WC.new_model(name, tmp_path)
    m.load_state_dict(WC.fixture_state(name, tmp_path), strict=True)
    return m.to(DEV).set_keep_activations(keep)


def _read(m, label, shape):
    return m.read_slot(m.backbone.labels[label], shape[1], shape[-2:]).cpu()


@pytest.mark.parametrize("name", ["C", "D"])
def test_layers_maps_decoder_and_head_match_the_reference(name, tmp_path):
    """Every labelled block tensor (stored for frame 1), the five feature maps, the decoder outputs and the head against the reference's own tensors; two forwards are
    bit-identical."""
    g = WC.golden(name)
    img = torch.from_numpy(g["frames"]).to(DEV)
    m = _model(name, tmp_path, keep=True)
    out = m(img)[HEAD].clone()
    torch.cuda.synchronize()
    worst, checked = 0.0, 0
    for key in sorted(k for k in g if k.startswith("layer/")):
        label = key[len("layer/"):]
        assert label in m.backbone.labels, label
        want = g[key]
        e = _err(_read(m, label, want.shape)[1:2], want)
        print(f"{label}: {e:.3g} (scale {np.abs(want).max():.3g})")
        assert e <= ATOL, (label, e)
        worst, checked = max(worst, e), checked + 1
    assert checked == 3 * sum(WC.FIXTURES[name]["depths"]) + 3
    for i, label in enumerate([f"{ENC}.embeddings"] + [f"{ENC}.stage{s}" for s in range(1, 5)]):
        e = _err(_read(m, label, g[f"feat/{i}"].shape), g[f"feat/{i}"])
        print(f"feat/{i}: {e:.3g}")
        assert e <= ATOL, (i, e)
        worst = max(worst, e)
    n_dec = sum(1 for k in g if k.startswith("dec/"))
    assert n_dec == 2
    for i in range(n_dec):
        want = g[f"dec/{i}"]
        e = _err(m.read_slot(m.backbone.decoder_slot_of_stride[int(g[f"dec_stride/{i}"])], want.shape[1], want.shape[-2:]).cpu(), want)
        print(f"dec/{i}: {e:.3g}")
        assert e <= ATOL, (i, e)
        worst = max(worst, e)
    e = _err(out.cpu(), g["head"])
    print(f"head: {e:.3g}; worst of fixture {name}: {max(worst, e):.3g}")
    assert out.shape == g["head"].shape and e <= ATOL
    again = m(img)[HEAD]
    torch.cuda.synchronize()
    assert torch.equal(again, out)


def test_window_24_model_matches_the_restatement_in_float64(tmp_path):
    """Fixture E: 576 tokens, 18 key tiles; stage 1 shifted by 12 on a 16x24 map (one window, mostly padded), stage 2 window 24 on 8x12, stage 3 window 12."""
    sd = WC.fixture_state("E", tmp_path)
    m = _model("E", tmp_path, keep=True)
    img = torch.from_numpy(WC.frames("E"))
    col = {}
    sd64 = {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
    want = R.model_forward(sd64, WC.backbone_config("E", "unused"), WC.arch_of("E"), WC.head_config("E"), "single_instance", img, collect=col)[HEAD]
    assert want.dtype == torch.float64
    got = m(img.to(DEV))[HEAD]
    torch.cuda.synchronize()
    worst = 0.0
    for label in (f"{ENC}.encoder.layers.0.blocks.0.attention.self", f"{ENC}.encoder.layers.0.blocks.1.attention.self", f"{ENC}.encoder.layers.0.blocks.1",
                  f"{ENC}.encoder.layers.1.blocks.0.attention.self", f"{ENC}.encoder.layers.2.blocks.0.attention.self", f"{ENC}.encoder.layers.3.blocks.0"):
        e = _err(_read(m, label, col[label].shape), col[label])
        print(f"{label}: {e:.3g}")
        assert e <= ATOL, (label, e)
        worst = max(worst, e)
    e = _err(got.cpu(), want)
    print(f"head: {e:.3g}; worst of fixture E: {max(worst, e):.3g}")
    assert got.shape == want.shape and e <= ATOL
    assert [(o.ksize, o.cmid) for o in m.ops if o.kind == 22] == WC.WINDOWS["E"]


def test_predictor_loads_a_run_directory(tmp_path):
    """``Predictor.from_model_paths([run_dir], pretrained_swinv2=True, swinv2_wide=True)`` on a run directory of fixture C gives the golden's peaks; without
    ``swinv2_wide`` the directory is refused and the message names the keyword."""
    from sleap_nn_amd.inference.predictor import Predictor

    g = WC.golden("C")
    run = WC.write_run_dir(tmp_path / "run_c", "C", WC.fixture_state("C", tmp_path))
    thr = float(g["peak_threshold"])
    rk, rv = O.single_instance_postprocess(torch.from_numpy(g["head"]), WC.FIXTURES["C"]["output_stride"], peak_threshold=thr)[:2]
    rk, rv = np.asarray(rk), np.asarray(rv)
    assert np.allclose(rk, g["peaks"], atol=1e-4) and not np.isnan(rk).any()
    with pytest.raises(NotImplementedError, match="swinv2_wide"):
        Predictor.from_model_paths([run], device=DEV, batch_size=2, peak_threshold=thr, pretrained_swinv2=True)
    with pytest.raises(NotImplementedError, match="pretrained_swinv2"):
        Predictor.from_model_paths([run], device=DEV, batch_size=2, peak_threshold=thr, swinv2_wide=True)
    p = Predictor.from_model_paths([run], device=DEV, batch_size=2, peak_threshold=thr, pretrained_swinv2=True, swinv2_wide=True)
    outs = p.predict(g["frames"])
    assert len(outs) == 1
    scale = max(1.0, float(np.abs(g["head"]).max()))
    k = outs[0].pred_keypoints.cpu().numpy().reshape(rk.shape)
    print(f"peaks: worst position error {np.abs(k - g['peaks'].reshape(rk.shape)).max():.3g} px")
    assert np.allclose(k, g["peaks"].reshape(rk.shape), atol=1e-4)
    assert np.allclose(outs[0].pred_peak_values.cpu().numpy().reshape(rv.shape), rv, atol=ATOL * scale)


@pytest.mark.parametrize("name", ["C", "D"])
def test_batch_of_one_equals_the_frame_inside_a_batch(name, tmp_path):
    g = WC.golden(name)
    img = torch.from_numpy(g["frames"])
    m = _model(name, tmp_path, keep=True)
    m.set_option("conv_wino4", 3)  # (the 3x3 kernel choice depends on the tile count, i.e. on the batch: one choice for the bitwise comparison, as in tests/test_gpu_pretrained_swinv2.py)
    m.set_option("conv_splitk", 0)
    m.set_option("conv_smallmap", 0)
    shape4 = g["feat/4"].shape
    both = m(img.to(DEV))[HEAD].clone()
    enc2 = _read(m, f"{ENC}.stage4", shape4)
    for b in (0, 1):
        one = m(img[b:b + 1].to(DEV))[HEAD]
        enc1 = _read(m, f"{ENC}.stage4", shape4)
        torch.cuda.synchronize()
        assert torch.equal(enc1, enc2[b:b + 1]) and torch.equal(one, both[b:b + 1]), b


@pytest.mark.parametrize("name", ["C", "D", "E"])
def test_kernel_routing_precisions_and_plan_invariant(name, tmp_path):
    """The default inference plan (slots recycled).  The kernel record shows the key-tiled kernel on every block whose window exceeds 8 (stages 1 and 2 of C and D) and the
    one-wave kernel on the others; ``set_precision("split" | "fp16")`` leaves outputs, kernels and ranges as they are; the recorded ranges satisfy the invariant of
    tests/test_gpu_plan_hazards.py, and the attention op's qkv source and its destination are on record."""
    from sleap_nn_amd import _lib as L
    from tests.test_gpu_plan_hazards import _check_plan

    img = torch.from_numpy(WC.frames(name)).to(DEV)
    m = _model(name, tmp_path)
    got = m(img)[HEAD].clone()
    torch.cuda.synchronize()
    _check_plan(m, f"pretrained swinv2 {name}")
    kv, rows = m.last_kernels(), m.last_ranges()
    seen = []
    for p, o in enumerate(m.ops):
        if o.kind == L.OP_WINDOW_ATTN_V2:
            assert kv[p] == (L.SWINV2_KV_WINDOW_ATTN_WIDE if o.ksize > 8 else L.SWINV2_KV_WINDOW_ATTN), (p, o.ksize, kv[p])
            seen.append(kv[p])
            assert any(op == p and not is_dst and slot == o.src0 for op, _ln, is_dst, slot, _o, _n in rows), p
            assert any(op == p and is_dst and slot == o.dst for op, _ln, is_dst, slot, _o, _n in rows), p
        elif o.kind == L.OP_LAYERNORM and o.flags & L.FLAG_RESIDUAL:
            assert kv[p] == L.SWINV2_KV_LAYERNORM_ADD
    wide, narrow = L.SWINV2_KV_WINDOW_ATTN_WIDE, L.SWINV2_KV_WINDOW_ATTN
    assert seen == {"C": [wide] * 4 + [narrow] * 2, "D": [wide] * 4 + [narrow] * 2, "E": [wide] * 4 + [narrow]}[name]
    for prec, kw in (("split", {}), ("fp16", {}), ("fp16", {"swint_f16": True})):
        m.set_precision(prec, **kw)
        again = m(img)[HEAD]
        torch.cuda.synchronize()
        assert torch.equal(again, got), (prec, kw)
        assert m.last_kernels() == kv and m.last_ranges() == rows, (prec, kw)


def test_training_is_refused_on_the_device(tmp_path):
    from sleap_nn_amd.training.module import TrainingModule

    m = _model("D", tmp_path)
    with pytest.raises(NotImplementedError, match="Swinv2"):
        m.train()
    with pytest.raises(NotImplementedError, match="Swinv2"):
        TrainingModule(m, pretrained_training=True)
