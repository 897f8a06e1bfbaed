"""GPU parity of the ``pretrained`` backbone's ResNet family (HuggingFace ResNetBackbone), inference, exact fp32, against the reference's own outputs
(tests/golden/pretrained_resnet*.npz: tools/gen_pretrained_resnet_golden.py) and, where there is no golden, against tests/resnet_ref.py (which
tests/test_pretrained_resnet_cpu.py holds to those outputs and to ``transformers``).

The bar is that of tests/test_gpu_pretrained.py: max error <= 1e-4 of max(1, scale).  Frames are 3 x 64 x 96; frame 1 is about 0.2 of the others' intensity.
Configuration A has bottleneck layers (reduced widths 8 .. 32, a projection shortcut at stride 1, identity shortcuts), B basic layers with widths that are no
multiples of 16.  Measured worst errors are in DESIGN 4.4g."""
import json

import numpy as np
import pytest
import torch

from oracle import cpu_ref as O
from tests import resnet_ref as R
from tests.test_pretrained_resnet_cpu import CONFIGS, RUN_DIR, bb_of, golden, heads_of, hf_dir, hf_json

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ATOL = 1e-4
HEAD = "SingleInstanceConfmapsHead"
ENC = "backbone.enc"


def _err(got, want):
    want = torch.as_tensor(want)
    return (got - want).abs().max().item() / max(1.0, want.abs().max().item())


def _model(name, tmp_path, sd=None, keep=False):
    from sleap_nn_amd.architectures.model import Model

    m = Model("pretrained", bb_of(name, hf_dir(name, tmp_path)), heads_of(name), "single_instance")
    m.load_state_dict(golden(name)[1] if sd is None else sd, strict=True)
    return m.to(DEV).set_keep_activations(keep)


def _random_model(tmp_path, arch, bb_over, heads, seed, keep=True):
    """A model over a config.json written here, with a random state (tests/resnet_ref.init_state) -> (model, state dict, backbone config)."""
    from sleap_nn_amd.architectures.model import Model

    d = tmp_path / f"hf_{seed}"
    d.mkdir(exist_ok=True)
    with open(d / "config.json", "w") as f:
        json.dump(hf_json(arch), f)
    bb = dict(bb_of("B", str(d)), **bb_over)
    m = Model("pretrained", bb, heads, "single_instance")
    sd = R.init_state(m.param_shapes, m.buffers, seed)
    m.load_state_dict(sd, strict=True)
    return m.to(DEV).set_keep_activations(keep), sd, bb


def _read(m, label, shape):
    return m.read_slot(m.backbone.labels[label], shape[1], shape[-2:]).cpu()


@pytest.mark.parametrize("name", ["A", "B"])
def test_layers_maps_decoder_and_head_match_the_reference(name, tmp_path):
    """Every labelled layer output, the five feature maps, the decoder outputs and the head against the reference's own tensors; two forwards are bit-identical."""
    g, _sd = golden(name)
    img = torch.from_numpy(g["frames"]).to(DEV)
    m = _model(name, tmp_path, keep=True)
    out = m(img)[HEAD].clone()
    torch.cuda.synchronize()
    worst, checked = 0.0, 0
    for key in sorted(k for k in g if k.startswith("layer/")):
        label = key[len("layer/"):]
        assert label in m.backbone.labels, label
        e = _err(_read(m, label, g[key].shape), g[key])
        print(f"{label}: {e:.3g} (scale {np.abs(g[key]).max():.3g})")
        assert e <= ATOL, (label, e)
        worst, checked = max(worst, e), checked + 1
    assert checked >= 15
    for i, label in enumerate([f"{ENC}.embedder"] + [f"{ENC}.stage{s}" for s in range(1, 5)]):
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
    print(f"head: {e:.3g}; worst of configuration {name}: {max(worst, e):.3g}")
    assert out.shape == g["head"].shape and e <= ATOL
    again = m(img)[HEAD]
    torch.cuda.synchronize()
    assert torch.equal(again, out)


def test_predictor_loads_the_run_directory():
    """``Predictor.from_model_paths([run_dir], pretrained_resnet=True)`` gives the peaks the oracle finds on the reference's head output (tolerances of the ConvNeXtV2
    run-directory test); without the keyword the directory is refused by name."""
    from sleap_nn_amd.inference.predictor import Predictor

    g, _sd = golden("A")
    thr = float(g["peak_threshold"])
    rk, rv = O.single_instance_postprocess(torch.from_numpy(g["head"]), CONFIGS["A"]["output_stride"], peak_threshold=thr)[:2]
    rk, rv = np.asarray(rk), np.asarray(rv)
    assert np.allclose(rk, g["peaks"], atol=1e-4) and not np.isnan(rk).any()
    with pytest.raises(NotImplementedError, match="pretrained_resnet"):
        Predictor.from_model_paths([RUN_DIR], device=DEV, batch_size=3, peak_threshold=thr)
    p = Predictor.from_model_paths([RUN_DIR], device=DEV, batch_size=3, peak_threshold=thr, pretrained_resnet=True)
    outs = p.predict(g["frames"])
    assert len(outs) == 1
    k = outs[0].pred_keypoints.cpu().numpy().reshape(rk.shape)
    assert np.allclose(k, rk, atol=1e-3)
    scale = max(1.0, float(np.abs(g["head"]).max()))
    assert np.allclose(outs[0].pred_peak_values.cpu().numpy().reshape(rv.shape), rv, atol=ATOL * scale)


@pytest.mark.parametrize("layer_type", ["bottleneck", "basic"])
def test_smallest_map(layer_type, tmp_path):
    """2 frames of 32 x 32: stage 4 is a 1 x 1 map, its 3x3 stride-2 conv has eight of nine taps outside the 2 x 2 map it reads."""
    arch = dict(CONFIGS["A" if layer_type == "bottleneck" else "B"])
    heads = {"confmaps": {"part_names": ["a", "b"], "sigma": 2.5, "output_stride": 4, "loss_weight": 1.0}}
    m, sd, bb = _random_model(tmp_path, arch, {"output_stride": 4, "normalize": True}, heads, seed=11)
    img = torch.randint(0, 256, (2, 3, 32, 32), dtype=torch.uint8, generator=torch.Generator().manual_seed(12))
    col = {}
    want = R.model_forward(sd, bb, heads, "single_instance", img, collect=col)[HEAD]
    got = m(img.to(DEV))[HEAD]
    torch.cuda.synchronize()
    last = f"{ENC}.encoder.stages.3.layers.0"
    assert col[last].shape[-2:] == (1, 1)
    for label in (f"{ENC}.embedder.embedder", f"{last}.shortcut", f"{last}.layer.1" if layer_type == "bottleneck" else f"{last}.layer.0", last):
        assert _err(_read(m, label, col[label].shape), col[label]) <= ATOL, label
    assert got.shape == want.shape and _err(got.cpu(), want) <= ATOL


def test_a_size_that_is_no_multiple_of_32_is_refused(tmp_path):
    m = _model("B", tmp_path)
    with pytest.raises(ValueError, match="multiples of 32"):
        m(torch.zeros(1, 3, 48, 80, dtype=torch.uint8, device=DEV))
    assert m(torch.zeros(1, 3, 64, 96, dtype=torch.uint8, device=DEV))[HEAD].shape == (1, 3, 16, 24)


@pytest.mark.parametrize("layer_type", ["bottleneck", "basic"])
def test_pad_channels_stay_zero(layer_type, tmp_path):
    """Widths 18 / 22 (bottleneck: reduced widths 4 / 5), embedding 12: the slots the new ops write have pad channels, all exactly zero, and the maps match the restatement."""
    from sleap_nn_amd import _lib as L

    arch = {"layer_type": layer_type, "embedding_size": 12, "hidden_sizes": [18, 22, 32, 48], "depths": [2, 1, 1, 1]}
    heads = {"confmaps": {"part_names": ["a", "b"], "sigma": 2.5, "output_stride": 8, "loss_weight": 1.0}}
    m, sd, bb = _random_model(tmp_path, arch, {"output_stride": 8, "filters_rate": 1.0, "normalize": True}, heads, seed=21)
    gen = torch.Generator().manual_seed(22)
    img = torch.randint(0, 256, (3, 3, 64, 96), dtype=torch.uint8, generator=gen)
    img[1] = (img[1].float() * 0.2).to(torch.uint8)
    col = {}
    want = R.model_forward(sd, bb, heads, "single_instance", img, collect=col)[HEAD]
    got = m(img.to(DEV))[HEAD]
    torch.cuda.synchronize()
    assert _err(got.cpu(), want) <= ATOL
    for label in (f"{ENC}.embedder.embedder", f"{ENC}.encoder.stages.0.layers.0.layer.1", f"{ENC}.encoder.stages.0.layers.1", f"{ENC}.encoder.stages.1.layers.0.shortcut",
                  f"{ENC}.encoder.stages.1.layers.0.layer.0", f"{ENC}.encoder.stages.1.layers.0.layer.1", f"{ENC}.encoder.stages.1.layers.0"):
        assert _err(_read(m, label, col[label].shape), col[label]) <= ATOL, label
    ws = m._workspace.view(torch.float32)
    where = {slot: (off, n) for _op, _ln, is_dst, slot, off, n in m.last_ranges() if is_dst and slot >= 0}
    new_kinds = (L.OP_RESNET_STEM, L.OP_CONV_S2, L.OP_ADD_RELU)
    seen = 0
    for o in m.ops:
        if not (o.kind in new_kinds or (o.kind == L.OP_LINEAR and o.flags & L.FLAG_RELU)):
            continue
        for slot in (o.dst, o.dst2):
            if slot < 0:
                continue
            cp = (o.cout + 15) // 16 * 16
            off, n = where[slot]
            t = ws[off // 4: (off + n) // 4]
            t = t[: t.numel() // cp * cp].view(-1, cp)
            if cp > o.cout:
                assert float(t[:, o.cout:].abs().max()) == 0.0, (o.label, slot)
                assert float(t[:, : o.cout].abs().max()) > 0.0
                seen += 1
    assert seen >= (10 if layer_type == "bottleneck" else 7)


def test_running_statistics_are_live(tmp_path):
    """Loading a second draw of running_mean / running_var moves the outputs to what the restatement gives for them (the fold is redone, the handle replaced)."""
    g, sd = golden("B")
    img = torch.from_numpy(g["frames"])
    m = _model("B", tmp_path)
    first = m(img.to(DEV))[HEAD].clone()
    gen0 = m.generation
    gen = torch.Generator().manual_seed(31)
    other = {k: (0.3 * torch.randn(v.shape, generator=gen) if k.endswith("running_mean") else (0.5 + 1.5 * torch.rand(v.shape, generator=gen)) if k.endswith("running_var") else v)
             for k, v in sd.items()}
    want = R.model_forward(other, bb_of("B", "unused"), heads_of("B"), "single_instance", img)[HEAD]
    assert _err(want, g["head"]) > 100 * ATOL
    m.load_state_dict(other, strict=True)
    assert m.generation > gen0  # anything that captured the old handle's pointers must not replay them
    got = m(img.to(DEV))[HEAD]
    torch.cuda.synchronize()
    assert _err(got.cpu(), want) <= ATOL and _err(first.cpu(), g["head"]) <= ATOL


def test_stem_pads_the_normalised_image(tmp_path):
    """normalize=True and a frame of constant value 0: the normalised image is -mean / std inside and 0 in the padding, so the stem map's border differs from its
    interior.  A kernel that pads before normalising gives one constant map."""
    m = _model("A", tmp_path, keep=True)
    _g, sd = golden("A")
    img = torch.zeros(1, 3, 64, 96, dtype=torch.uint8)
    col = {}
    R.model_forward(sd, bb_of("A", "unused"), heads_of("A"), "single_instance", img, collect=col)
    want = col[f"{ENC}.embedder.embedder"]
    inner = want[0, :, 8, 8]
    assert float((want[0, :, 2:-2, 2:-2] - inner.view(-1, 1, 1)).abs().max()) < 1e-5 and float((want[0, :, 0, 0] - inner).abs().max()) > 1e-2
    m(img.to(DEV))
    got = _read(m, f"{ENC}.embedder.embedder", want.shape)
    assert _err(got, want) <= ATOL
    assert float((got[0, :, 0, 0] - got[0, :, 8, 8]).abs().max()) > 1e-2


@pytest.mark.parametrize("name", ["A", "B"])
def test_batch_of_one_equals_the_frame_inside_a_batch(name, tmp_path):
    g, _sd = golden(name)
    img = torch.from_numpy(g["frames"])
    m = _model(name, tmp_path, keep=True)
    m.set_option("conv_wino4", 3)  # (the 3x3 kernel choice depends on the tile count, i.e. on the batch: one choice for the bitwise comparison, as in tests/test_gpu_pretrained.py)
    m.set_option("conv_splitk", 0)
    m.set_option("conv_smallmap", 0)
    shape4 = g["feat/4"].shape
    all3 = m(img.to(DEV))[HEAD].clone()
    enc3 = _read(m, f"{ENC}.stage4", shape4)
    for b in (0, 1):
        one = m(img[b:b + 1].to(DEV))[HEAD]
        enc1 = _read(m, f"{ENC}.stage4", shape4)
        torch.cuda.synchronize()
        assert torch.equal(enc1, enc3[b:b + 1]) and torch.equal(one, all3[b:b + 1]), b


@pytest.mark.parametrize("name", ["A", "B"])
def test_precisions_routes_and_plan_invariant(name, tmp_path):
    """The default inference plan (slots recycled): ``set_precision("split" | "fp16")``, with or without the ``*_f16`` options, leaves the program exact; the kernel
    record names the new variants for the stem, the strided convs and the add and an existing conv route for every stride-1 3x3; the recorded ranges satisfy the
    invariant of tests/test_gpu_plan_hazards.py, with the stem's two launches on record."""
    from sleap_nn_amd import _lib as L
    from tests.test_gpu_plan_hazards import _check_plan

    g, _sd = golden(name)
    img = torch.from_numpy(g["frames"]).to(DEV)
    m = _model(name, tmp_path)
    got = m(img)[HEAD].clone()
    torch.cuda.synchronize()
    assert _err(got.cpu(), g["head"]) <= ATOL
    _check_plan(m, f"pretrained resnet {name}")
    kv, rows = m.last_kernels(), m.last_ranges()
    conv_routes = (L.KV_DIRECT, L.KV_WINO1D, L.KV_WINO2D, L.KV_W16, L.KV_C16, L.KV_ROWGEMM, L.KV_WINO4, L.KV_WINO2D_KS, L.KV_SMALLMAP)
    n_s2 = n_conv = 0
    for p, o in enumerate(m.ops):
        if o.kind == L.OP_RESNET_STEM:
            assert kv[p] == L.RESNET_KV_STEM
            mine = [(ln, is_dst, slot) for op, ln, is_dst, slot, _o, _n in rows if op == p]
            assert sorted(mine) == sorted([(0, True, o.dst), (1, False, o.dst), (1, True, o.dst2)]), mine
        elif o.kind == L.OP_CONV_S2:
            assert kv[p] == L.RESNET_KV_CONV_S2
            n_s2 += 1
        elif o.kind == L.OP_ADD_RELU:
            assert kv[p] == L.RESNET_KV_ADD_RELU
        elif o.kind == L.OP_LINEAR:
            assert kv[p] == L.KV_ROWGEMM
            if o.flags & L.FLAG_RESIDUAL:
                assert o.flags & L.FLAG_RELU and any(op == p and not is_dst and slot == o.src1 for op, _ln, is_dst, slot, _o, _n in rows), p
        elif o.kind == L.OP_CONV and (o.weight or "").startswith(ENC):
            assert kv[p] in conv_routes, (p, kv[p])
            n_conv += 1
    assert n_s2 == 6 and n_conv >= 3 and (L.RESNET_KV_ADD_RELU in kv) == (name == "B")  # three strided stages: a 3x3 and a shortcut each
    for prec, kw in (("split", {}), ("fp16", {}), ("fp16", {"convnext_f16": True}), ("fp16", {"swint_f16": True})):
        m.set_precision(prec, **kw)
        again = m(img)[HEAD]
        torch.cuda.synchronize()
        assert torch.equal(again, got), (prec, kw)
        assert m.last_kernels()[0] == L.RESNET_KV_STEM


def test_training_is_refused_on_the_device(tmp_path):
    """``Model.train()``, ``TrainingModule(model)`` and ``ph_model_backward`` itself refuse the program, naming the backbone."""
    import ctypes as C

    from sleap_nn_amd import _lib as L
    from sleap_nn_amd.training.module import TrainingModule

    m = _model("B", tmp_path, keep=True)
    with pytest.raises(NotImplementedError, match="ResNet"):
        m.train()
    with pytest.raises(NotImplementedError, match="ResNet"):
        TrainingModule(m, pretrained_training=True)
    g, _sd = golden("B")
    img = torch.from_numpy(g["frames"]).to(DEV)
    m.set_option("pretrained_train", 1)  # (what lifts the ConvNeXtV2 refusal does not lift this one)
    out = m(img)[HEAD]
    B, _c, H, W = img.shape
    lib = L.lib()
    gws = torch.empty(1 << 20, dtype=torch.uint8, device=DEV)  # (the refusal comes before any plan is made: the size does not matter)
    loss, grads, tgt = torch.zeros(2, device=DEV), torch.zeros(m.num_parameters(), device=DEV), torch.zeros_like(out)
    outs, tgts = (C.c_void_p * 1)(out.data_ptr()), (C.c_void_p * 1)(tgt.data_ptr())
    rc = lib.ph_model_backward(m._handle, C.c_void_p(img.data_ptr()), 0, B, 3, H, W, C.c_void_p(m._workspace.data_ptr()), C.c_void_p(gws.data_ptr()), gws.numel(), outs, tgts,
                               (C.c_float * 1)(1.0), None, 0, 2.0, 2, 2 ** 31 - 1, 5.0, C.c_void_p(loss.data_ptr()), C.c_void_p(grads.data_ptr()), L.current_stream_ptr())
    assert rc != 0 and "ResNet" in lib.ph_last_error().decode()
