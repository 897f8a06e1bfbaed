"""GPU parity of the ``pretrained`` (HuggingFace ConvNeXtV2) backbone, inference, exact fp32, against the reference's own outputs
(tests/golden/pretrained_convnextv2*.npz: tools/gen_pretrained_golden.py) and, per labelled block, against tests/convnextv2_ref.py (which
tests/test_pretrained_cpu.py holds to those outputs and to ``transformers``).

The bar is that of tests/test_gpu_convnext.py / test_gpu_swint.py: max error <= 1e-4 of max(1, scale).  Frames are 3 x 64 x 96: stage 1 has 384 pixels per
sample, so the 256-row GEMM tiles (32-row blocks in the fused plan's epilogue) and GRN's fixed slices meet sample boundaries; stage 4 has 6 pixels per sample, several samples in one tile; frame 1
is about 0.2 of the others' intensity, so a reduction that spans the batch changes the answer.  Configuration B has widths that are no multiples of 16."""
import numpy as np
import pytest
import torch

from oracle import cpu_ref as O
from tests import convnextv2_ref as R
from tests.test_pretrained_cpu import CONFIGS, RUN_DIR, bb_of, golden, heads_of, hf_dir

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ATOL = 1e-4
HEAD = "SingleInstanceConfmapsHead"


def _err(got, want):
    want = torch.as_tensor(want)
    return (got - want).abs().max().item() / max(1.0, want.abs().max().item())


def _model(name, tmp_path, sd=None, keep=False, fuse=0):
    from sleap_nn_amd.architectures.model import Model

    m = Model("pretrained", bb_of(name, hf_dir(name, tmp_path)), heads_of(name), "single_instance")
    m.load_state_dict(golden(name)[1] if sd is None else sd, strict=True)
    m.to(DEV).set_keep_activations(keep)
    m.set_option("grn_fuse", fuse)
    return m


_REF = {}


def _ref(name):
    """convnextv2_ref's labelled activations of a configuration, computed once."""
    if name not in _REF:
        g, sd = golden(name)
        collect = {}
        R.model_forward(sd, bb_of(name, "unused"), heads_of(name), "single_instance", torch.from_numpy(g["frames"]), collect=collect)
        _REF[name] = collect
    return _REF[name]


@pytest.mark.parametrize("fuse", [0, 1])
@pytest.mark.parametrize("name", ["A", "B"])
def test_blocks_and_heads_match_the_reference(name, fuse, tmp_path):
    """Every labelled block (stem, GRN outputs, block outputs, the four normed maps, decoder convs) and the head output, on the two-launch GRN (``grn_fuse`` 0) and
    on the fused plan (1: the GRN output never exists there, its labels are left out); two forwards are bit-identical on either."""
    from sleap_nn_amd import _lib as L

    g, _sd = golden(name)
    img = torch.from_numpy(g["frames"]).to(DEV)
    m = _model(name, tmp_path, keep=True, fuse=fuse)
    out = m(img)[HEAD].clone()
    torch.cuda.synchronize()
    kv = list(m.last_kernels())
    n_blocks = sum(CONFIGS[name]["depths"])
    assert kv.count(L.CNX2_KV_GRN_FUSED if fuse else L.CNX2_KV_GRN) == n_blocks and kv.count(L.CNX2_KV_GRN if fuse else L.CNX2_KV_GRN_FUSED) == 0
    assert kv[0] == L.CNX2_KV_PATCH_STEM_NORM
    checked = 0
    for label, t in _ref(name).items():
        assert label in m.backbone.labels, label
        if fuse and label.endswith(".grn"):
            checked += 1
            continue
        got = m.read_activation(label, t.shape[0], t.shape[-2:]).cpu()
        e = _err(got, t)
        print(f"{label}: {e:.3g} (scale {t.abs().max().item():.3g})")
        assert e <= ATOL, (label, e)
        checked += 1
    assert checked >= 2 * sum(CONFIGS[name]["depths"]) + 5 + 2 * 3
    for i in range(1, 5):  # the reference's own maps (golden), not only the restatement's
        got = m.read_activation(f"backbone.enc.hidden_states_norms.stage{i}", 3, g[f"feat/{i}"].shape[-2:]).cpu()
        assert _err(got, g[f"feat/{i}"]) <= ATOL, i
    e = _err(out.cpu(), g["head"])
    print(f"head: {e:.3g}")
    assert out.shape == g["head"].shape and e <= ATOL
    again = m(img)[HEAD]
    torch.cuda.synchronize()
    assert torch.equal(again, out)


@pytest.mark.parametrize("name", ["A", "B"])
def test_fused_and_unfused_plans_agree(name, tmp_path):
    """The default inference plan (slots recycled) with ``grn_fuse`` 1 against 0, to the parity bar; the fused one passes the plan invariant with its scratch uses on
    record (block sums written by the first Linear and read by the finalize launch, weight images written and read by the second Linear's two launches) and the
    residual Linear reading the GELU output itself; the option round-trips through ``ph_model_set_option`` / ``ph_model_get_option``."""
    from sleap_nn_amd import _lib as L
    from tests.test_gpu_plan_hazards import _check_plan

    g, _sd = golden(name)
    img = torch.from_numpy(g["frames"]).to(DEV)
    m = _model(name, tmp_path)
    plain = m(img)[HEAD].clone()
    torch.cuda.synchronize()
    assert m.get_option("grn_fuse") == 0.0  # the default
    m.set_option("grn_fuse", 1)
    assert m.get_option("grn_fuse") == 1.0
    fused = m(img)[HEAD].clone()
    torch.cuda.synchronize()
    assert L.CNX2_KV_GRN_FUSED in m.last_kernels() and L.CNX2_KV_GRN not in m.last_kernels()
    assert _err(fused.cpu(), g["head"]) <= ATOL and _err(fused.cpu(), plain.cpu()) <= ATOL
    assert not torch.equal(fused, plain)  # (another order of operations: the two plans are not the same launches)
    _check_plan(m, f"pretrained {name} fused")
    rows = m.last_ranges()
    for p, o in enumerate(m.ops):
        if o.kind == L.OP_GRN:
            mine = lambda q: [(ln, is_dst, slot) for op, ln, is_dst, slot, _o, _n in rows if op == q]  # noqa: E731
            assert (0, True, -1) in mine(p - 1) and (0, False, -1) in mine(p) and (0, True, o.dst) in mine(p), p
            assert (0, False, o.dst) in mine(p + 1) and (0, True, -1) in mine(p + 1) and (1, False, -1) in mine(p + 1) and (1, False, o.src0) in mine(p + 1), p
    again = m(img)[HEAD]
    torch.cuda.synchronize()
    assert torch.equal(again, fused)
    m.set_option("grn_fuse", 0)
    back = m(img)[HEAD]
    torch.cuda.synchronize()
    assert m.get_option("grn_fuse") == 0.0 and torch.equal(back, plain)


def test_hidden_width_with_pad_channels(tmp_path):
    """C = 18 / 22: the hidden tensors have 72 / 88 channels in 80 / 96 padded ones, so GRN's channel mean runs over the true channels only and its pad outputs are
    zeros (the fixtures' 4C widths are all multiples of 16).  Random weights, against convnextv2_ref, both plans."""
    import json

    from sleap_nn_amd.architectures.model import Model

    d = tmp_path / "hf_pad"
    d.mkdir()
    with open(d / "config.json", "w") as f:
        json.dump({"model_type": "convnextv2", "depths": [1, 1, 1, 1], "hidden_sizes": [18, 22, 32, 48], "patch_size": 4, "num_channels": 3, "hidden_act": "gelu"}, f)
    bb = dict(bb_of("B", str(d)), filters_rate=1.0, output_stride=8)
    heads = {"confmaps": {"part_names": ["a", "b"], "sigma": 2.5, "output_stride": 8, "loss_weight": 1.0}}
    m = Model("pretrained", bb, heads, "single_instance")
    gen = torch.Generator().manual_seed(77)
    sd = {}
    for k, shape in m.param_shapes.items():
        if ".grn." in k:
            sd[k] = 0.5 * torch.randn(shape, generator=gen)
        elif "norm" in k or ".downsampling_layer.0." in k:
            sd[k] = (1.0 if k.endswith(".weight") else 0.0) + 0.5 * torch.randn(shape, generator=gen)
        elif len(shape) > 1:
            sd[k] = torch.randn(shape, generator=gen) * (2.0 / (shape[0] + shape[1] * int(np.prod(shape[2:])))) ** 0.5
        else:
            sd[k] = 0.2 * (torch.rand(shape, generator=gen) * 2 - 1)
    sd.update(m.buffers)
    m.load_state_dict(sd, strict=True)
    m.to(DEV).set_keep_activations(True)
    img = torch.randint(0, 256, (3, 3, 64, 96), dtype=torch.uint8, generator=gen)
    img[1] = (img[1].float() * 0.2).to(torch.uint8)
    collect = {}
    want = R.model_forward(sd, bb, heads, "single_instance", img, collect=collect)[HEAD]
    for fuse in (0, 1):
        m.set_option("grn_fuse", fuse)
        got = m(img.to(DEV))[HEAD]
        torch.cuda.synchronize()
        assert _err(got.cpu(), want) <= ATOL, fuse
        for label in ("backbone.enc.encoder.stages.0.layers.0", "backbone.enc.encoder.stages.1.layers.0") + (() if fuse else ("backbone.enc.encoder.stages.0.layers.0.grn",)):
            t = collect[label]
            assert _err(m.read_activation(label, 3, t.shape[-2:]).cpu(), t) <= ATOL, (fuse, label)


@pytest.mark.parametrize("name", ["A", "B"])
def test_recycling_plan_precisions_and_plan_invariant(name, tmp_path):
    """The default inference plan (slots recycled) gives the same maps, passes the no-overlap / liveness invariant of tests/test_gpu_plan_hazards.py with GRN's two
    launches and their scratch on record, and ``set_precision("split" | "fp16")`` -- with ``convnext_f16`` set, too -- leaves the program exact."""
    from sleap_nn_amd import _lib as L
    from tests.test_gpu_plan_hazards import _check_plan

    g, _sd = golden(name)
    img = torch.from_numpy(g["frames"]).to(DEV)
    m = _model(name, tmp_path)
    got = m(img)[HEAD].clone()
    torch.cuda.synchronize()
    assert _err(got.cpu(), g["head"]) <= ATOL
    _check_plan(m, f"pretrained {name}")
    rows = m.last_ranges()
    for p, o in enumerate(m.ops):
        if o.kind == L.OP_GRN:  # launch 0 writes the scratch region, launch 1 reads it and writes the op's slot
            mine = [(ln, is_dst, slot) for op, ln, is_dst, slot, _o, _n in rows if op == p]
            assert (0, True, -1) in mine and (1, False, -1) in mine and (1, True, o.dst) in mine and (0, False, o.src0) in mine and (1, False, o.src0) in mine, (p, mine)
        if o.kind == L.OP_LINEAR and o.flags & L.FLAG_RESIDUAL:
            assert any(op == p and not is_dst and slot == o.src1 for op, _ln, is_dst, slot, _o, _n in rows), p
    for prec, f16 in (("split", None), ("fp16", None), ("fp16", True)):
        m.set_precision(prec, convnext_f16=f16)
        again = m(img)[HEAD]
        torch.cuda.synchronize()
        assert torch.equal(again, got), (prec, f16)
        assert L.CNX2_KV_GRN in m.last_kernels() and L.CNX_KV_F16_GEMM not in m.last_kernels()


def test_grn_is_seen(tmp_path):
    """With GRN's weight and bias zeroed (HuggingFace's initial values: GRN is then the identity) the output leaves the golden far behind."""
    g, sd = golden("A")
    z = {k: (torch.zeros_like(v) if ".grn." in k else v) for k, v in sd.items()}
    m = _model("A", tmp_path, sd=z)
    out = m(torch.from_numpy(g["frames"]).to(DEV))[HEAD]
    torch.cuda.synchronize()
    assert _err(out.cpu(), g["head"]) > 100 * ATOL


def test_batch_of_one_and_gray_frames(tmp_path):
    """B = 1 and B = 3 give the same first (and second, dim) frame, bit for bit on the two-launch GRN: nothing reduces across samples.  A 1-channel frame is replicated to three."""
    g, sd = golden("A")
    img = torch.from_numpy(g["frames"])
    m = _model("A", tmp_path, keep=True)
    m.set_option("conv_wino4", 3)  # (the decoder's 3x3 kernel choice depends on the tile count, i.e. on the batch: one choice for the bitwise comparison, as in tests/test_gpu_swint.py)
    m.set_option("conv_splitk", 0)
    m.set_option("conv_smallmap", 0)
    hw4 = g["feat/4"].shape[-2:]
    for fuse in (0, 1):
        m.set_option("grn_fuse", fuse)
        all3 = m(img.to(DEV))[HEAD].clone()
        enc3 = m.read_activation("backbone.enc.hidden_states_norms.stage4", 3, hw4).clone()
        for b in (0, 1):
            one = m(img[b:b + 1].to(DEV))[HEAD]
            enc1 = m.read_activation("backbone.enc.hidden_states_norms.stage4", 1, hw4)
            torch.cuda.synchronize()
            assert _err(one.cpu(), g["head"][b:b + 1]) <= ATOL, (fuse, b)
            if fuse == 0 or b == 0:  # the two-launch GRN cuts its sums per sample: bit for bit whatever the batch.  The fused plan's sums are per 32-row block of the whole
                assert torch.equal(enc1, enc3[b:b + 1]), (fuse, b)  # batch, so where a sample's rows start inside a block (sample 1 at 24 pixels per sample) they are added
                assert torch.equal(one, all3[b:b + 1]), (fuse, b)   # in another order than alone: equal to the bar there, bit for bit only for sample 0
            else:
                assert _err(enc1.cpu(), enc3[b:b + 1].cpu()) <= ATOL and _err(one.cpu(), all3[b:b + 1].cpu()) <= ATOL, (fuse, b)
    m.set_option("grn_fuse", 0)
    gray = img[:, :1].contiguous()
    want = R.model_forward(sd, bb_of("A", "unused"), heads_of("A"), "single_instance", gray)[HEAD]
    got = m(gray.to(DEV))[HEAD]
    torch.cuda.synchronize()
    assert _err(got.cpu(), want) <= ATOL


def test_float_input_and_checkpoint_statistics(tmp_path):
    """Float frames in [0, 1] take the same path; image statistics other than the config's, read from the checkpoint, are the ones applied."""
    g, sd = golden("A")
    img = torch.from_numpy(g["frames"])
    m = _model("A", tmp_path)
    got = m((img.float() / 255.0).to(DEV))[HEAD]
    torch.cuda.synchronize()
    assert _err(got.cpu(), g["head"]) <= ATOL
    other = dict(sd)
    other["backbone.image_mean"] = torch.tensor([0.3, 0.5, 0.2]).view(1, 3, 1, 1)
    other["backbone.image_std"] = torch.tensor([0.4, 0.15, 0.3]).view(1, 3, 1, 1)
    want = R.model_forward(other, bb_of("A", "unused"), heads_of("A"), "single_instance", img)[HEAD]
    assert _err(want, g["head"]) > 100 * ATOL
    got = _model("A", tmp_path, sd=other)(img.to(DEV))[HEAD]
    torch.cuda.synchronize()
    assert _err(got.cpu(), want) <= ATOL


def test_training_is_refused_on_the_device(tmp_path):
    from sleap_nn_amd.training.module import TrainingModule

    m = _model("A", tmp_path)
    with pytest.raises(NotImplementedError, match="pretrained"):
        m.train()
    with pytest.raises(NotImplementedError, match="pretrained"):
        TrainingModule(m)


def test_predictor_loads_the_run_directory():
    """best.ckpt + training_config.yaml (``model_name: hf_config``, next to the checkpoint) -> Predictor.from_model_paths -> the peaks the oracle finds on the
    reference's head output; tolerances as tests/test_gpu_swint.py has them for keypoints and peak values."""
    from sleap_nn_amd.inference.predictor import Predictor

    g, _sd = golden("A")
    thr = float(g["peak_threshold"])
    rk, rv = O.single_instance_postprocess(torch.from_numpy(g["head"]), CONFIGS["A"]["output_stride"], peak_threshold=thr)[:2]
    rk, rv = np.asarray(rk), np.asarray(rv)
    assert np.allclose(rk, g["peaks"], atol=1e-4) and not np.isnan(rk).any()
    p = Predictor.from_model_paths([RUN_DIR], device=DEV, batch_size=3, peak_threshold=thr)
    outs = p.predict(g["frames"])
    assert len(outs) == 1
    k = outs[0].pred_keypoints.cpu().numpy().reshape(rk.shape)
    assert np.allclose(k, rk, atol=1e-3)
    scale = max(1.0, float(np.abs(g["head"]).max()))
    assert np.allclose(outs[0].pred_peak_values.cpu().numpy().reshape(rv.shape), rv, atol=ATOL * scale)
