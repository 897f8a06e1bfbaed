"""GPU parity of the ``pretrained`` backbone's Swinv2 family (HuggingFace Swinv2Backbone), inference, exact fp32, against the reference's own outputs
(tests/golden/pretrained_swinv2_*.npz: tools/gen_pretrained_swinv2_golden.py) and, where there is no golden, against tests/swinv2_ref.py (which
tests/test_pretrained_swinv2_cpu.py holds to those outputs and to ``transformers``).  The weights are drawn from the golden's seed (tests/_swinv2_cases.py).

The bar is that of the other pretrained families: max error <= 1e-4 of max(1, scale) per map.  Fixture A (window 4, frames 96 x 160: stages 3 and 4 pad their
windows, stage 3 runs unshifted, stage 4 at window 2), fixture B (window 7: two token tiles with dead key columns, pretrained_window_sizes 6, frames 96 x 128), and a
window-8 model (64 tokens exactly).  Frame 1 is about 0.2 of frame 0's intensity.  Measured worst errors are in DESIGN 4.4h."""
import numpy as np
import pytest
import torch

from oracle import cpu_ref as O
from tests import _swinv2_cases as SC
from tests import swinv2_ref as R
from tests.test_pretrained_swinv2_cpu import ENC, HEAD, arch_of, bb_of, golden, golden_state, heads_of, new_model, state_of, write_run_dir

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ATOL = 1e-4


def _err(got, want):
    want = torch.as_tensor(want)
    return (got - want).abs().max().item() / max(1.0, want.abs().max().item())


def _model(name, tmp_path, sd=None, keep=False):
    m = new_model(name, tmp_path)
    m.load_state_dict(golden_state(name, tmp_path) if sd is None else sd, strict=True)
    return m.to(DEV).set_keep_activations(keep)


def _read(m, label, shape):
    return m.read_slot(m.backbone.labels[label], shape[1], shape[-2:]).cpu()


@pytest.mark.parametrize("name", ["A", "B"])
def test_layers_maps_decoder_and_head_match_the_reference(name, tmp_path):
    """Every labelled block tensor (the attention branch back on the map, x1, the block output, the merge outputs; stored for frame 1), the five feature maps, the decoder
    outputs and the head against the reference's own tensors; the tensors the golden does not hold (attention core, MLP halves, reduction) against the restatement;
    two forwards are bit-identical."""
    g, sd = golden(name), golden_state(name, tmp_path)
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
    assert checked == 3 * sum(SC.FIXTURES[name]["depths"]) + 3
    col = {}
    R.model_forward(sd, bb_of(name, "unused"), arch_of(name), heads_of(name), "single_instance", torch.from_numpy(g["frames"]), collect=col)
    extra = [k for k in col if k.endswith((".attention.self", ".intermediate", ".output", ".reduction")) or k.endswith("patch_embeddings.projection")]
    assert len(extra) == 3 * sum(SC.FIXTURES[name]["depths"]) + 3 + 1
    for label in extra:
        e = _err(_read(m, label, col[label].shape), col[label])
        print(f"{label} (restatement): {e:.3g}")
        assert e <= ATOL, (label, e)
        worst = max(worst, e)
    for i, label in enumerate([f"{ENC}.embeddings"] + [f"{ENC}.stage{s}" for s in range(1, 5)]):
        e = _err(_read(m, label, g[f"feat/{i}"].shape), g[f"feat/{i}"])
        print(f"feat/{i}: {e:.3g}")
        assert e <= ATOL, (i, e)
        worst = max(worst, e)
    n_dec = sum(1 for k in g if k.startswith("dec/"))
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


def test_window_8_model_matches_the_restatement(tmp_path):
    """Window 8: N = 64 exactly, both token tiles full; stage 4 unshifted as in the published window8-256 models."""
    c = SC.FIXTURES["W8"]
    m = new_model("W8", tmp_path)
    sd = state_of(m, c["seed"])
    m.load_state_dict(sd, strict=True)
    m.to(DEV).set_keep_activations(True)
    img = torch.from_numpy(SC.frames("W8"))
    col = {}
    want = R.model_forward(sd, bb_of("W8", "unused"), arch_of("W8"), heads_of("W8"), "single_instance", img, collect=col)[HEAD]
    got = m(img.to(DEV))[HEAD]
    torch.cuda.synchronize()
    for label in (f"{ENC}.encoder.layers.0.blocks.0.attention.self", f"{ENC}.encoder.layers.0.blocks.1.attention.self", f"{ENC}.encoder.layers.0.blocks.1",
                  f"{ENC}.encoder.layers.1.blocks.1", f"{ENC}.encoder.layers.3.blocks.0"):
        e = _err(_read(m, label, col[label].shape), col[label])
        print(f"{label}: {e:.3g}")
        assert e <= ATOL, (label, e)
    assert got.shape == want.shape and _err(got.cpu(), want) <= ATOL
    assert [(o.ksize, o.cmid) for o in m.ops if o.kind == 22] == [(8, 0), (8, 4), (8, 0), (8, 4), (8, 0), (8, 0)]


def test_predictor_loads_a_run_directory(tmp_path):
    """``Predictor.from_model_paths([run_dir], pretrained_swinv2=True)`` on a run directory written here from the seeded state gives the peaks the oracle finds on the
    reference's head output; without the keyword the directory is refused by name."""
    from sleap_nn_amd.inference.predictor import Predictor

    g = golden("A")
    run = write_run_dir(tmp_path / "run_a", "A", golden_state("A", tmp_path))
    thr = float(g["peak_threshold"])
    rk, rv = O.single_instance_postprocess(torch.from_numpy(g["head"]), SC.FIXTURES["A"]["output_stride"], peak_threshold=thr)[:2]
    rk, rv = np.asarray(rk), np.asarray(rv)
    assert np.allclose(rk, g["peaks"], atol=1e-4) and not np.isnan(rk).any()
    with pytest.raises(NotImplementedError, match="pretrained_swinv2"):
        Predictor.from_model_paths([run], device=DEV, batch_size=2, peak_threshold=thr)
    p = Predictor.from_model_paths([run], device=DEV, batch_size=2, peak_threshold=thr, pretrained_swinv2=True)
    outs = p.predict(g["frames"])
    assert len(outs) == 1
    k = outs[0].pred_keypoints.cpu().numpy().reshape(rk.shape)
    assert np.allclose(k, rk, atol=1e-3)
    scale = max(1.0, float(np.abs(g["head"]).max()))
    assert np.allclose(outs[0].pred_peak_values.cpu().numpy().reshape(rv.shape), rv, atol=ATOL * scale)


@pytest.mark.parametrize("name", ["A", "B"])
def test_smallest_frame(name, tmp_path):
    """2 frames of 32 x 32: maps 8x8 / 4x4 / 2x2 / 1x1 -- every window of stages 2 to 4 is mostly padded tokens, and a shifted layer rolls a map one window covers."""
    sd = golden_state(name, tmp_path)
    m = _model(name, tmp_path, keep=True)
    img = torch.randint(0, 256, (2, 3, 32, 32), dtype=torch.uint8, generator=torch.Generator().manual_seed(12))
    col = {}
    want = R.model_forward(sd, bb_of(name, "unused"), arch_of(name), heads_of(name), "single_instance", img, collect=col)[HEAD]
    got = m(img.to(DEV))[HEAD]
    torch.cuda.synchronize()
    last = f"{ENC}.encoder.layers.3.blocks.0"
    assert col[last].shape[-2:] == (1, 1)
    for label in (f"{ENC}.encoder.layers.1.blocks.1.attention.self", f"{ENC}.encoder.layers.2.blocks.1", f"{ENC}.encoder.layers.2.downsample", last + ".attention.self", last):
        e = _err(_read(m, label, col[label].shape), col[label])
        assert e <= ATOL, (label, e)
    assert got.shape == want.shape and _err(got.cpu(), want) <= ATOL


def test_a_size_that_is_no_multiple_of_32_is_refused(tmp_path):
    m = _model("B", tmp_path)
    with pytest.raises(ValueError, match="multiples of 32"):
        m(torch.zeros(1, 3, 48, 80, dtype=torch.uint8, device=DEV))
    assert m(torch.zeros(1, 3, 64, 96, dtype=torch.uint8, device=DEV))[HEAD].shape == (1, 3, 8, 12)


@pytest.mark.parametrize("name", ["A", "B"])
def test_batch_of_one_equals_the_frame_inside_a_batch(name, tmp_path):
    g = golden(name)
    img = torch.from_numpy(g["frames"])
    m = _model(name, tmp_path, keep=True)
    m.set_option("conv_wino4", 3)  # (the 3x3 kernel choice depends on the tile count, i.e. on the batch: one choice for the bitwise comparison, as in tests/test_gpu_pretrained.py)
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


@pytest.mark.parametrize("name", ["A", "B"])
def test_precisions_routes_and_plan_invariant(name, tmp_path):
    """The default inference plan (slots recycled): ``set_precision("split" | "fp16")``, with or without ``swint_f16`` / ``convnext_f16``, leaves outputs, kernels and
    ranges as they are; the kernel record names the new variants; the recorded ranges satisfy the invariant of tests/test_gpu_plan_hazards.py (the residual LayerNorm's
    shortcut is on record as a source)."""
    from sleap_nn_amd import _lib as L
    from tests.test_gpu_plan_hazards import _check_plan

    g = golden(name)
    img = torch.from_numpy(g["frames"]).to(DEV)
    m = _model(name, tmp_path)
    got = m(img)[HEAD].clone()
    torch.cuda.synchronize()
    assert _err(got.cpu(), g["head"]) <= ATOL
    _check_plan(m, f"pretrained swinv2 {name}")
    kv, rows = m.last_kernels(), m.last_ranges()
    n_att = 0
    for p, o in enumerate(m.ops):
        if o.kind == L.OP_WINDOW_ATTN_V2:
            assert kv[p] == L.SWINV2_KV_WINDOW_ATTN
            n_att += 1
        elif o.kind == L.OP_LAYERNORM and o.flags & L.FLAG_RESIDUAL:
            assert kv[p] == L.SWINV2_KV_LAYERNORM_ADD
            assert any(op == p and not is_dst and slot == o.src1 for op, _ln, is_dst, slot, _o, _n in rows), p
        elif o.kind == L.OP_PATCH_MERGE:
            assert kv[p] == L.SWINV2_KV_MERGE_GATHER
        elif o.kind == L.OP_LINEAR:
            assert kv[p] == L.KV_ROWGEMM
        elif o.kind == L.OP_PATCH_STEM:
            assert kv[p] == L.CNX2_KV_PATCH_STEM_NORM
    assert n_att == sum(SC.FIXTURES[name]["depths"])
    for prec, kw in (("split", {}), ("fp16", {}), ("fp16", {"swint_f16": True}), ("fp16", {"convnext_f16": True}), ("split", {"swint_f16": True})):
        m.set_precision(prec, **kw)
        again = m(img)[HEAD]
        torch.cuda.synchronize()
        assert torch.equal(again, got), (prec, kw)
        assert m.last_kernels() == kv and m.last_ranges() == rows, (prec, kw)


def test_training_is_refused_on_the_device(tmp_path):
    """``Model.train()``, ``TrainingModule(model)`` and ``ph_model_backward`` itself refuse the program, naming the backbone."""
    import ctypes as C

    from sleap_nn_amd import _lib as L
    from sleap_nn_amd.training.module import TrainingModule

    m = _model("B", tmp_path, keep=True)
    with pytest.raises(NotImplementedError, match="Swinv2"):
        m.train()
    with pytest.raises(NotImplementedError, match="Swinv2"):
        TrainingModule(m, pretrained_training=True)
    img = torch.from_numpy(golden("B")["frames"]).to(DEV)
    m.set_option("pretrained_train", 1)  # (what lifts the ConvNeXtV2 refusal does not lift this one)
    out = m(img)[HEAD]
    B, _c, H, W = img.shape
    lib = L.lib()
    gws = torch.empty(1 << 20, dtype=torch.uint8, device=DEV)  # (the refusal comes before any plan is made: the size does not matter)
    loss, grads, tgt = torch.zeros(2, device=DEV), torch.zeros(m.num_parameters(), device=DEV), torch.zeros_like(out)
    outs, tgts = (C.c_void_p * 1)(out.data_ptr()), (C.c_void_p * 1)(tgt.data_ptr())
    rc = lib.ph_model_backward(m._handle, C.c_void_p(img.data_ptr()), 0, B, 3, H, W, C.c_void_p(m._workspace.data_ptr()), C.c_void_p(gws.data_ptr()), gws.numel(), outs, tgts,
                               (C.c_float * 1)(1.0), None, 0, 2.0, 2, 2 ** 31 - 1, 5.0, C.c_void_p(loss.data_ptr()), C.c_void_p(grads.data_ptr()), L.current_stream_ptr())
    assert rc != 0 and "Swinv2" in lib.ph_last_error().decode()


def test_derived_forms_are_rebuilt_on_load(tmp_path):
    """Reloading the same checkpoint changes nothing, bit for bit (the derived qkv bias keeps its zero key section); a changed ``logit_scale`` or bias-MLP weight moves
    the output to what the restatement gives for it: the derived forms are made again from what was loaded."""
    g, sd = golden("A"), golden_state("A", tmp_path)
    img = torch.from_numpy(g["frames"])
    m = _model("A", tmp_path)
    first = m(img.to(DEV))[HEAD].clone()
    gen0 = m.generation
    m.load_state_dict(sd, strict=True)
    same = m(img.to(DEV))[HEAD].clone()
    torch.cuda.synchronize()
    assert m.generation > gen0 and torch.equal(same, first)
    d = m.backbone.derived_params(m._state, m.buffers)
    assert all(float(v[v.numel() // 3: 2 * v.numel() // 3].abs().max()) == 0.0 for k, v in d.items() if k.endswith("query.bias"))
    bb, arch = bb_of("A", "unused"), arch_of("A")
    for suffix, change in (("blocks.0.attention.self.logit_scale", lambda v: v - 1.0), ("continuous_position_bias_mlp.0.weight", lambda v: -v)):
        other = {k: (change(v) if k.endswith(suffix) else v) for k, v in sd.items()}
        want = R.model_forward(other, bb, arch, heads_of("A"), "single_instance", img)[HEAD]
        assert _err(want, g["head"]) > 10 * ATOL, suffix
        m.load_state_dict(other, strict=True)
        got = m(img.to(DEV))[HEAD]
        torch.cuda.synchronize()
        assert _err(got.cpu(), want) <= ATOL, suffix
    assert _err(first.cpu(), g["head"]) <= ATOL
