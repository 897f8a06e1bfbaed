"""Training a ``pretrained`` (HuggingFace ConvNeXtV2) backbone on the device: forward + MSE + backward (GRN backward, the weight gradient of the padding-0
normalised patch stem, and the ConvNeXt / decoder steps that were there) against torch autograd over tests/convnextv2_ref.py's ``model_forward``; frozen
encoder, unread parameters, Adam / AdamW against torch's optimizers.

Bars (those of the ConvNeXt and Swin training tests): loss within 1e-5 relative, every parameter gradient within 2e-4 of its tensor's largest magnitude.  On the CPU,
golden config A at 2 x 3 x 64 x 96: torch's fp32 autograd sits at most 1.2e-6 of scale from its float64 autograd, and every read parameter has a non-zero gradient.

Image seeds come from a CPU scan (SEEDS): a decoder ReLU whose pre-activation lies inside the forward's error takes the other branch of its kink on the device and
moves every gradient upstream of it, which is no property of the kernels.  Every case prints the reference's smallest |ReLU pre-activation| next to the device's
largest error on the decoder maps and asserts a factor of ten between them.  (Seed 5 on config A comes within 7.8e-6.)
"""
import json

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import convnextv2_ref as R
from tests.test_pretrained_cpu import CONFIGS, bb_of, golden, heads_of, hf_dir

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
LOSS_RTOL = 1e-5
GRAD_BAR = 2e-4
MT = "single_instance"
HEAD = "SingleInstanceConfmapsHead"
STEM_NORM = ("backbone.enc.hidden_states_norms.stem.weight", "backbone.enc.hidden_states_norms.stem.bias")
STEM_W = "backbone.enc.embeddings.patch_embeddings.weight"
# image seed per case, from the CPU scan of the reference's smallest |ReLU pre-activation| (seeds 0..59, 0..79 for the frozen three-step case; the values found are printed by the case)
SEEDS = {"A": 7, "pad": 18, "dead": 18, "wide": 55, "float": 7, "gray": 46, "convt": 0, "os8": 57, "adam": 7, "frozen": 78, "seg": 0}


def _img(shape, seed):
    return torch.randint(0, 256, shape, dtype=torch.uint8, generator=torch.Generator().manual_seed(seed))


def _hf_dir(tmp_path, hidden, depths=(1, 1, 1, 1)):
    d = tmp_path / ("hf_" + "_".join(str(h) for h in hidden))
    d.mkdir(exist_ok=True)
    with open(d / "config.json", "w") as f:
        json.dump({"model_type": "convnextv2", "depths": list(depths), "hidden_sizes": list(hidden), "patch_size": 4, "num_channels": 3, "hidden_act": "gelu"}, f)
    return str(d)


def _rand_state(m, seed):
    """Random weights as tests/test_gpu_pretrained.py draws them: GRN parameters and norm affines away from their initial values."""
    gen = torch.Generator().manual_seed(seed)
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
    return sd


def _ref_step(sd, bb, heads, img, targets, frozen=False, mt=MT):
    """nn.MSELoss per head (weight 1) + autograd over convnextv2_ref.model_forward -> (loss, {name: gradient}, outputs, labelled maps,
    {decoder map: smallest |pre-activation| of its ReLU}, names without a gradient).  The stem norm is read by nobody (nor is a stage norm whose map the decoder does not take): its gradient is None on this side and
    reported as zeros.  ``frozen``: the encoder parameters are detached."""
    names = [k for k, v in sd.items() if v.is_floating_point() and not k.startswith("backbone.image_")]
    params = {k: sd[k].clone().requires_grad_(not (frozen and k.startswith("backbone.enc."))) for k in names}
    relu, margin, collect = F.relu, [], {}

    def watched(x, *a, **k):
        margin.append(float(x.detach().abs().min()))
        return relu(x, *a, **k)

    F.relu = watched
    try:
        out = R.model_forward({**sd, **params}, bb, heads, mt, img, collect=collect)
    finally:
        F.relu = relu
    loss = sum(F.mse_loss(out[k], targets[k]) for k in out)
    loss.backward()
    unread = sorted(k for k, p in params.items() if p.grad is None)  # (frozen: the encoder's too)
    assert set(STEM_NORM) <= set(unread)
    grads = {k: (torch.zeros_like(p) if p.grad is None else p.grad.detach()) for k, p in params.items()}
    relu_maps = [k for k in collect if k.startswith("backbone.dec.")]  # one labelled map per ReLU of the reference, in call order
    assert len(relu_maps) == len(margin)
    return float(loss.detach()), grads, {k: v.detach() for k, v in out.items()}, {k: v.detach() for k, v in collect.items()}, dict(zip(relu_maps, margin)), unread


def _errors(got, ref):
    assert set(got) == set(ref), set(got) ^ set(ref)
    return {k: float((got[k].cpu() - r).abs().max()) / max(float(r.abs().max()), 1e-12) for k, r in ref.items()}


def _check(tm, loss, ref):
    """Loss and every gradient to the bars; the kink margin against the device's error on the decoder maps."""
    ref_loss, ref_grads, _out, collect, margin, unread = ref
    torch.cuda.synchronize()
    got = tm.named_grads()
    assert all(torch.isfinite(g).all() for g in got.values())
    errs = _errors(got, ref_grads)
    worst = sorted(errs.items(), key=lambda kv: -kv[1])[:4]
    B = next(iter(collect.values())).shape[0]
    print("loss", float(loss[0]), ref_loss, "worst", worst)
    close = {}
    for label, least in margin.items():
        fwd = float((tm.model.read_activation(label, B, collect[label].shape[-2:]).cpu() - collect[label]).abs().max())
        print("%s: smallest |ReLU pre-activation| of the reference %.3g, device error on the map %.3g" % (label.split(".")[-1], least, fwd))
        if least < 10 * fwd:
            close[label] = (least, fwd)
    assert not close, close
    assert abs(float(loss[0]) - ref_loss) <= LOSS_RTOL * max(1.0, abs(ref_loss))
    bad = {k: v for k, v in errs.items() if v > GRAD_BAR}
    assert not bad, sorted(bad.items(), key=lambda kv: -kv[1])[:8]
    # what autograd leaves without a gradient is what the optimizer's ranges leave out, and its device gradient is exactly zero
    o, outside = 0, []
    for k in tm.model.param_keys():
        n = got[k].numel()
        if not any(lo <= o and o + n <= hi for lo, hi in tm._ranges):
            outside.append(k)
        o += n
    assert sorted(outside) == unread, set(outside) ^ set(unread)
    for k in unread:
        assert float(got[k].abs().max()) == 0.0, k
    return got


def _module(bb, heads, sd, mt=MT, **kw):
    from sleap_nn_amd.architectures.model import Model
    from sleap_nn_amd.training.module import TrainingModule

    m = Model("pretrained", bb, heads, mt)
    m.load_state_dict(sd, strict=True)
    kw.setdefault("loss_weights", [1.0])
    return TrainingModule(m, DEV, pretrained_training=True, **kw)


def _targets(sd, bb, heads, img, seed, mt=MT):
    with torch.no_grad():
        shapes = {k: v.shape for k, v in R.model_forward(sd, bb, heads, mt, img).items()}
    g = torch.Generator().manual_seed(seed + 100)
    return {k: torch.rand(s, generator=g) * 0.5 for k, s in shapes.items()}


def _case(bb, heads, sd, img, seed=0, frozen=False, **module_kw):
    targets = _targets(sd, bb, heads, img, seed)
    ref = _ref_step(sd, bb, heads, img, targets, frozen=frozen)
    tm = _module(bb, heads, sd, **module_kw)
    loss = tm.forward_backward(img.to(DEV), {k: v.to(DEV) for k, v in targets.items()})
    got = _check(tm, loss, ref)
    return tm, targets, ref, got


_A = {}


def _case_a(tmp_path):
    """Case 1's inputs and reference step, computed once."""
    if not _A:
        _g, sd = golden("A")
        img = _img((2, 3, 64, 96), SEEDS["A"])
        bb, heads = bb_of("A", "unused"), heads_of("A")
        targets = _targets(sd, bb, heads, img, 1)
        _A.update(sd=sd, img=img, heads=heads, targets=targets, ref=_ref_step(sd, bb, heads, img, targets))
    return dict(_A, bb=bb_of("A", hf_dir("A", tmp_path)))


def test_golden_config_all_gradients_and_backward_route(tmp_path):
    """Config A ([16, 32, 48, 64], depths [1, 1, 2, 1]), B = 2, uint8: stage 1 has 384 pixels per sample = two GRN slices (256 + 128), stage 4 has 6.  Loss and every
    gradient to the bars, the stem-norm gradients exactly zero, the GRN backward reported once per block and on no other op; a second pass is bit-identical."""
    from sleap_nn_amd import _lib as L

    a = _case_a(tmp_path)
    tm = _module(a["bb"], a["heads"], a["sd"])
    dev_t = {k: v.to(DEV) for k, v in a["targets"].items()}
    loss = tm.forward_backward(a["img"].to(DEV), dev_t)
    _check(tm, loss, a["ref"])
    assert all(float(g.abs().max()) > 0 for k, g in a["ref"][1].items() if k not in STEM_NORM)
    codes = tm.model.last_backward_kernels()
    assert codes.count(L.CNX2_KV_GRN_BWD) == sum(CONFIGS["A"]["depths"])
    assert all((c == L.CNX2_KV_GRN_BWD) == (o.kind == L.OP_GRN) for c, o in zip(codes, tm.model.ops))
    assert tm.frozen_encoder is False and tm.model.get_option("bwd_frozen_ops") == 0.0 and tm.model.get_option("pretrained_train") == 1.0
    g1 = tm.grads.clone()
    tm.forward_backward(a["img"].to(DEV), dev_t)
    torch.cuda.synchronize()
    assert torch.equal(tm.grads, g1)
    # without the handle option the C ABI keeps refusing the program
    tm.model.set_option("pretrained_train", 0)
    with pytest.raises(L.PosehipError, match="pretrained_train"):
        tm.forward_backward(a["img"].to(DEV), dev_t)
    tm.close()


def _pad_model(tmp_path, hidden, **bbkw):
    from sleap_nn_amd.architectures.model import Model

    bb = dict(bb_of("B", _hf_dir(tmp_path, hidden)), filters_rate=1.0, output_stride=8)
    bb.update(bbkw)
    heads = {"confmaps": {"part_names": ["a", "b"], "sigma": 2.5, "output_stride": bb["output_stride"], "loss_weight": 1.0}}
    return bb, heads, _rand_state(Model("pretrained", bb, heads, MT), 77)


def test_hidden_width_with_pad_channels(tmp_path):
    """hidden_sizes [18, 22, 32, 48]: 4C = 72 / 88 in 80 / 96 padded channels -- 20 channel quads, so the reduction's 12 rows do not divide a slice and 16 of its
    threads idle; the pad channels' gradients are zeros, never NaN, and nothing downstream of them is."""
    _case(*_pad_model(tmp_path, [18, 22, 32, 48]), _img((2, 3, 64, 96), SEEDS["pad"]), seed=2)


def test_dead_hidden_channel(tmp_path):
    """One row of a pwconv1.weight and its bias zeroed: that hidden channel is exactly zero behind the GELU, G = 0, K = 0; autograd's gradient there is finite."""
    _g, sd = golden("A")
    sd = dict(sd)
    k = "backbone.enc.encoder.stages.0.layers.0.pwconv1"
    sd[k + ".weight"] = sd[k + ".weight"].clone()
    sd[k + ".bias"] = sd[k + ".bias"].clone()
    sd[k + ".weight"][5] = 0
    sd[k + ".bias"][5] = 0
    _tm, _t, ref, got = _case(bb_of("A", hf_dir("A", tmp_path)), heads_of("A"), sd, _img((2, 3, 64, 96), SEEDS["dead"]), seed=3)
    gw = k.replace("pwconv1", "grn") + ".weight"
    assert float(ref[1][gw][..., 5].abs().max()) == 0.0 and float(got[gw][..., 5].abs().max()) == 0.0  # T = sum g x = 0 there
    assert float(ref[1][k + ".weight"][5].abs().max()) > 0  # ... while dx = g passes through it (1 + w N = 1, x K = 0) and GELU'(0) = 0.5


def test_last_stage_with_two_channel_chunks(tmp_path):
    """A last stage of 272 channels: 4C = 1088 = 272 quads, two 256-quad chunks of the reduction (the second with 16 quads x 16 rows) on a 2 x 3 map."""
    _case(*_pad_model(tmp_path, [16, 32, 48, 272]), _img((2, 3, 64, 96), SEEDS["wide"]), seed=4)


@pytest.mark.parametrize("kind", ["unit", "byte", "gray"])
def test_input_forms_reach_the_stem_weight_gradient(kind, tmp_path):
    """Float frames in [0, 1] (dtype code 1), float frames in [0, 255] (code 2) and a one-channel uint8 frame, which is replicated to three channels before the
    forward AND the backward see it.  The stem's weight gradient is to the bar in each (with every other gradient)."""
    _g, sd = golden("A")
    img = _img((2, 1 if kind == "gray" else 3, 64, 96), SEEDS["gray" if kind == "gray" else "float"])
    x = {"unit": img.float() / 255.0, "byte": img.float(), "gray": img}[kind]
    _tm, _t, ref, got = _case(bb_of("A", hf_dir("A", tmp_path)), heads_of("A"), sd, x, seed=5)
    scale = float(ref[1][STEM_W].abs().max())
    err = float((got[STEM_W] - ref[1][STEM_W]).abs().max()) / scale
    print(kind, "stem weight gradient: error %.3g of scale %.3g" % (err, scale))
    assert scale > 0 and err <= GRAD_BAR


def test_transposed_conv_decoder(tmp_path):
    _case(*_pad_model(tmp_path, [16, 32, 48, 64], up_interpolate=False, output_stride=4, filters_rate=1.5), _img((2, 3, 64, 96), SEEDS["convt"]), seed=6)


def test_output_stride_8_fewer_decoder_blocks(tmp_path):
    _case(*_pad_model(tmp_path, [16, 32, 48, 64], output_stride=8, filters_rate=2.0), _img((2, 3, 64, 96), SEEDS["os8"]), seed=7)


def test_batch_16_crop0_invariant_and_bitwise_repeatable(tmp_path):
    """B = 16.  Every crop but crop 0 gets its own prediction as target (its output gradient is exactly zero): B times the batch's gradients are crop 0's own, to the
    bar -- the sample-order sums of dw and dbeta, the per-sample dx; two identical steps give bitwise identical gradient arenas."""
    _g, sd = golden("A")
    B = 16
    img = _img((B, 3, 64, 96), 16)
    tm = _module(bb_of("A", hf_dir("A", tmp_path)), heads_of("A"), sd)
    out = tm.model.forward(img.to(DEV))[HEAD].clone()
    tgt = out.clone()
    tgt[0] = torch.rand(tgt[0].shape, generator=torch.Generator().manual_seed(5)).to(DEV) * 0.5
    tm.forward_backward(img.to(DEV), {HEAD: tgt})
    g16 = tm.grads.clone()
    named16 = tm.named_grads()
    tm.forward_backward(img.to(DEV), {HEAD: tgt})
    torch.cuda.synchronize()
    assert torch.equal(tm.grads, g16)
    tm.forward_backward(img[:1].to(DEV), {HEAD: tgt[:1]})
    torch.cuda.synchronize()
    named1 = tm.named_grads()
    errs = _errors({k: v * B for k, v in named16.items()}, named1)
    bad = {k: v for k, v in errs.items() if v > GRAD_BAR}
    assert not bad, sorted(bad.items(), key=lambda kv: -kv[1])[:8]
    assert all(float(named1[k].abs().max()) > 0 for k in named1 if k not in STEM_NORM)


def test_grn_fuse_does_not_reach_the_training_program(tmp_path):
    """``grn_fuse`` = 1 set before training: the training program is the unfused one, its forward reports the two-launch GRN, and the gradients are those of case 1,
    bit for bit those of the same module with the option at 0."""
    from sleap_nn_amd import _lib as L

    a = _case_a(tmp_path)
    dev_t = {k: v.to(DEV) for k, v in a["targets"].items()}
    tm = _module(a["bb"], a["heads"], a["sd"])
    tm.model.set_option("grn_fuse", 1)
    loss = tm.forward_backward(a["img"].to(DEV), dev_t)
    _check(tm, loss, a["ref"])
    assert tm.model.get_option("grn_fuse") == 1.0
    kv = tm.model.last_kernels()
    assert kv.count(L.CNX2_KV_GRN) == sum(CONFIGS["A"]["depths"]) and L.CNX2_KV_GRN_FUSED not in kv
    fused = tm.grads.clone()
    tm.model.set_option("grn_fuse", 0)
    tm.forward_backward(a["img"].to(DEV), dev_t)
    torch.cuda.synchronize()
    assert torch.equal(tm.grads, fused)
    tm.close()


def _movement_check(got, opt_params, tiny, lr_steps):
    over = {}
    for k, p in opt_params.items():
        d = (got[k].cpu() - p.detach()).abs()
        big = d[~tiny[k]]
        strict, loose = (float(big.max()) if big.numel() else 0.0) / lr_steps, float(d.max()) / lr_steps
        if strict > 0.02 or loose > 0.10:
            over[k] = (round(strict, 4), round(loose, 4))
    print("worst movement differences (share of 3 x lr; entries with a non-tiny gradient, all entries):", sorted(over.items(), key=lambda kv: -kv[1][1])[:12])
    return over


def test_three_adam_steps_match_reference_optimizer(tmp_path):
    """Three steps against torch.optim.Adam driven by the reference gradients; the entry-wise movement bars of the Swin and ConvNeXt tests (2 % of 3 x lr where the
    gradient is not tiny, 10 % everywhere), with their precautions: ``wgrad_wino`` = 0 keeps exactly-zero weight gradients of dead decoder channels exact, and the image
    seed keeps the smallest ReLU pre-activation of all three reference steps away from the forward's error.  The loss goes down; the stem norm does not move."""
    _g, sd = golden("A")
    bb, heads = bb_of("A", hf_dir("A", tmp_path)), heads_of("A")
    img = _img((2, 3, 64, 96), SEEDS["adam"])
    tm, targets, _ref, _got = _case(bb, heads, sd, img, seed=8, wino4=False)
    tm.model.set_option("wgrad_wino", 0)
    floats = {k: v for k, v in sd.items() if v.is_floating_point() and not k.startswith("backbone.image_")}
    opt_params = {k: torch.nn.Parameter(v.clone()) for k, v in floats.items()}
    opt = torch.optim.Adam(list(opt_params.values()), lr=1e-3)
    tm.lr = 1e-3
    batch = {"image": img.to(DEV), **{k: v.to(DEV) for k, v in targets.items()}}
    first, margins = None, []
    tiny = {k: torch.zeros_like(v, dtype=torch.bool) for k, v in floats.items()}
    for _step in range(3):
        _l, grads, _o, _c, margin, _u = _ref_step({**sd, **{k: p.detach() for k, p in opt_params.items()}}, bb, heads, img, targets)
        margins.append(margin)
        for k, p in opt_params.items():
            p.grad = None if k in STEM_NORM else grads[k]  # torch leaves an unread parameter's .grad at None and its optimizers skip it
            tiny[k] |= (grads[k].abs() < 1e-3 * grads[k].abs().max()) & (grads[k] != 0)
        opt.step()
        loss = tm.training_step(batch)
        first = float(loss[0]) if first is None else first
    torch.cuda.synchronize()
    print("smallest |ReLU pre-activation| of the three reference steps:", [min(m.values()) for m in margins])
    got = tm.state_dict()
    over = _movement_check(got, opt_params, tiny, 3e-3)
    assert float(loss[0]) < first
    assert not over, sorted(over.items(), key=lambda kv: -kv[1][1])[:8]
    assert sum(int(t.sum()) for t in tiny.values()) < 0.5 * sum(t.numel() for t in tiny.values())
    for k in STEM_NORM:
        assert torch.equal(got[k], sd[k]), k
    tm.close()


def test_frozen_encoder_three_adamw_steps(tmp_path):
    """``freeze_encoder=True``, three AdamW steps with weight_decay 0.01: every ``backbone.enc.*`` tensor of the state dict is the loaded one, its gradient exactly
    zero, no encoder op ran a backward step; decoder and head gradients meet the bars against autograd with the encoder parameters detached; the decoder moves as
    torch.optim.AdamW moves it.  Unfrozen, the two stem-norm tensors are likewise untouched by AdamW's decay.  The config's ``freeze: true`` means the same."""
    from sleap_nn_amd import _lib as L

    _g, sd = golden("A")
    bb, heads = bb_of("A", hf_dir("A", tmp_path)), heads_of("A")
    img = _img((2, 3, 64, 96), SEEDS["frozen"])
    tm, targets, ref, got = _case(bb, heads, sd, img, seed=9, frozen=True, freeze_encoder=True, optimizer="AdamW", weight_decay=0.01, wino4=False)
    tm.model.set_option("wgrad_wino", 0)
    enc = [k for k in tm.model.param_keys() if k.startswith("backbone.enc.")]
    assert tm.frozen_encoder and len(enc) > 40
    for k in enc:
        assert float(got[k].abs().max()) == 0.0, k
    n_enc = tm.model.backbone.encoder_ops()
    codes = tm.model.last_backward_kernels()
    assert tm.model.get_option("bwd_frozen_ops") == float(n_enc) and all(c == L.KV_NONE for c in codes[:n_enc])
    assert all(float(got[k].abs().max()) > 0 for k in got if k not in enc)
    dec = {k: v for k, v in sd.items() if v.is_floating_point() and not k.startswith("backbone.image_") and k not in enc}
    opt_params = {k: torch.nn.Parameter(v.clone()) for k, v in dec.items()}
    opt = torch.optim.AdamW(list(opt_params.values()), lr=1e-3, weight_decay=0.01)
    tm.lr = 1e-3
    batch = {"image": img.to(DEV), **{k: v.to(DEV) for k, v in targets.items()}}
    tiny = {k: torch.zeros_like(v, dtype=torch.bool) for k, v in dec.items()}
    first = None
    for _step in range(3):
        _l, grads, *_ = _ref_step({**sd, **{k: p.detach() for k, p in opt_params.items()}}, bb, heads, img, targets, frozen=True)
        for k, p in opt_params.items():
            p.grad = grads[k]
            tiny[k] |= (grads[k].abs() < 1e-3 * grads[k].abs().max()) & (grads[k] != 0)
        opt.step()
        loss = tm.training_step(batch)
        first = float(loss[0]) if first is None else first
    torch.cuda.synchronize()
    state = tm.state_dict()
    for k in enc:
        assert torch.equal(state[k], sd[k]), k
    assert float(tm.grads[: tm._ranges[0][0]].abs().max()) == 0.0 and float(loss[0]) < first
    assert not _movement_check(state, opt_params, tiny, 3e-3)
    tm.close()
    # unfrozen under AdamW: the stem norm, which no op reads, neither decays nor moves; a read encoder parameter does move
    tm2 = _module(bb, heads, sd, optimizer="AdamW", weight_decay=0.01)
    for _step in range(3):
        tm2.training_step(batch)
    torch.cuda.synchronize()
    state2 = tm2.state_dict()
    for k in STEM_NORM:
        assert torch.equal(state2[k], sd[k]), k
    assert not torch.equal(state2[STEM_W], sd[STEM_W])
    tm2.close()
    # the backbone config's own `freeze: true`
    tm3 = _module(dict(bb, freeze=True), heads, sd)
    assert tm3.frozen_encoder and tm3.model.get_option("bwd_frozen_ops") == float(n_enc)
    tm3.forward_backward(batch["image"], targets)
    torch.cuda.synchronize()
    got3 = tm3.named_grads()
    assert all(float(got3[k].abs().max()) == 0.0 for k in enc) and tm3.model.last_backward_kernels()[:n_enc] == [L.KV_NONE] * n_enc
    errs = _errors({k: v for k, v in got3.items() if k not in enc}, {k: v for k, v in ref[1].items() if k not in enc})
    assert max(errs.values()) <= GRAD_BAR, errs
    tm3.close()
    assert _module(dict(bb, freeze=True), heads, sd, freeze_encoder=False).frozen_encoder is False  # the keyword overrides the config


def test_bucket_event_fires_with_the_split_op_frozen(tmp_path):
    """The arena's clean split of config A lies inside the encoder.  With the encoder frozen and a bucket event bound, the backward still records it (the gradient
    exchange of a data-parallel run waits on it), and the gradients are those of the run without an event."""
    from sleap_nn_amd import _lib as L

    a = _case_a(tmp_path)
    dev_t = {k: v.to(DEV) for k, v in a["targets"].items()}
    tm = _module(a["bb"], a["heads"], a["sd"], freeze_encoder=True)
    tm.forward_backward(a["img"].to(DEV), dev_t)
    plain = tm.grads.clone()
    split = int(L.check(L.lib().ph_model_grad_bucket_split(tm.model._handle)))
    assert 0 < split < tm._ranges[0][0]  # the split parameter belongs to a frozen op
    e0, ev, e1 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
    ev.record()  # creates the underlying event; this record is the stale one
    torch.cuda.synchronize()
    tm._bucket_event = ev
    e0.record()
    tm.forward_backward(a["img"].to(DEV), dev_t)
    e1.record()
    torch.cuda.synchronize()
    assert e0.elapsed_time(ev) > 0 and ev.elapsed_time(e1) >= 0  # recorded again by this backward: behind its start, not behind its end
    assert torch.equal(tm.grads, plain)
    tm.close()


def test_eval_after_a_training_step(tmp_path):
    """After a training step and eval(): the inference forward of the trained handle equals that of a fresh model loaded from tm.state_dict(), on the two-launch GRN
    and on the fused plan, whose folded bias W2 grn.bias + b2 follows the parameters."""
    from sleap_nn_amd.architectures.model import Model

    a = _case_a(tmp_path)
    tm = _module(a["bb"], a["heads"], a["sd"], lr=1e-3)
    loss = tm.training_step({"image": a["img"].to(DEV), **{k: v.to(DEV) for k, v in a["targets"].items()}})
    torch.cuda.synchronize()
    assert torch.isfinite(loss).all()
    tm.model.eval()  # the handle of the inference program is created from the model's host copy, which is stale here, and takes the live arena through ph_model_set_params
    got = {}
    for fuse in (0, 1):
        tm.model.set_option("grn_fuse", fuse)
        got[fuse] = tm.model(a["img"][:1].to(DEV))[HEAD].clone()
    state = tm.state_dict()
    gk = "backbone.enc.encoder.stages.2.layers.1.grn.bias"
    assert not torch.equal(state[gk], a["sd"][gk])
    fresh = Model("pretrained", a["bb"], a["heads"], MT)
    fresh.load_state_dict(state, strict=True)
    fresh.to(DEV)
    for fuse in (0, 1):
        fresh.set_option("grn_fuse", fuse)
        want = fresh(a["img"][:1].to(DEV))[HEAD]
        torch.cuda.synchronize()
        assert torch.equal(got[fuse], want), fuse
    assert not torch.equal(got[0], got[1])
    tm.close()


def test_segmentation_training_module_takes_the_keyword(tmp_path):
    """A ``semantic_segmentation`` model on this backbone through SegmentationTrainingModule(pretrained_training=True): finite loss, every read parameter's
    gradient non-zero; without the keyword it refuses by name."""
    from sleap_nn_amd.architectures.model import Model
    from sleap_nn_amd.training.segmentation import SegmentationTrainingModule

    bb = bb_of("A", hf_dir("A", tmp_path))
    heads = {"segmentation": {"output_stride": 2, "loss_weight": 1.0}}
    m = Model("pretrained", bb, heads, "semantic_segmentation")
    m.load_state_dict(_rand_state(m, 12), strict=True)
    with pytest.raises(NotImplementedError, match="pretrained_training"):
        SegmentationTrainingModule(m, DEV)
    tm = SegmentationTrainingModule(m, DEV, pretrained_training=True)
    img = _img((2, 3, 64, 96), SEEDS["seg"])
    yy, xx = torch.meshgrid(torch.arange(32), torch.arange(48), indexing="ij")
    mask = (((xx - 20) ** 2 + (yy - 14) ** 2) <= 81).float().expand(2, 1, 32, 48).contiguous()
    loss = tm.forward_backward(img, {"SegmentationHead": mask})
    torch.cuda.synchronize()
    assert torch.isfinite(loss).all() and float(loss[0]) > 0
    got = tm.named_grads()
    assert all(torch.isfinite(g).all() for g in got.values())
    assert all((float(g.abs().max()) > 0) == (k not in STEM_NORM) for k, g in got.items())
    tm.close()
