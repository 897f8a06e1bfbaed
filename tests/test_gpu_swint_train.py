"""Training a Swin Transformer backbone on the device: forward + MSE + backward (window-attention backward, patch-merge backward, residual fan-out,
per-sample branch scales) against torch autograd over tests/swin_ref.py's ``model_forward``.

Bars (those of the ConvNeXt training tests, tests/test_gpu_convnext.py): loss within 1e-5 relative, every parameter gradient within 2e-4 of its tensor's
largest magnitude, the same set of gradient names on both sides.  The reference's own fp32 autograd sits 1.8e-6 .. 2.9e-6 of scale from its float64
autograd on the first three shapes below (worst: the bias tables), about 70 times inside the bar.
"""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from tests import swin_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
LOSS_RTOL = 1e-5
GRAD_BAR = 2e-4
SMALL = {"embed": 32, "depths": [2, 2, 2, 2], "num_heads": [1, 2, 4, 8]}
MT = "single_instance"
HEAD = "SingleInstanceConfmapsHead"


def _bb(**kw):
    bb = {"model_type": None, "arch": SMALL, "in_channels": 1, "patch_size": 4, "window_size": 7, "kernel_size": 3, "filters_rate": 2, "convs_per_block": 2,
          "up_interpolate": True, "stem_patch_stride": 2, "output_stride": 2, "max_stride": 32, "pre_trained_weights": None}
    bb.update(kw)
    return bb


def _heads(n, stride=2):
    return {"confmaps": {"part_names": [str(i) for i in range(n)], "sigma": 2.5, "output_stride": stride, "loss_weight": 1.0, "anchor_part": None}}


def _img(shape, seed):
    return torch.randint(0, 256, shape, dtype=torch.uint8, generator=torch.Generator().manual_seed(seed))


def _ref_step(sd, bb, heads, mt, img, targets):
    """nn.MSELoss per head (weight 1) + autograd over swin_ref.model_forward -> (loss, {name: gradient}) for every float entry of the state."""
    params = {k: v.clone().requires_grad_(True) for k, v in sd.items() if v.is_floating_point()}
    relu, margin = F.relu, []

    def watched(x, *a, **k):  # a pre-activation closer to zero than the forward's error puts the two sides on different branches of the kink: print how close the case comes
        margin.append(float(x.detach().abs().min()))
        return relu(x, *a, **k)

    F.relu = watched
    try:
        out = R.model_forward({**sd, **params}, bb, heads, mt, img)
    finally:
        F.relu = relu
    print("smallest |ReLU pre-activation| of the reference: %.3g" % min(margin))
    loss = sum(F.mse_loss(out[k], targets[k]) for k in out)
    loss.backward()
    assert all(p.grad is not None for p in params.values())
    return float(loss.detach()), {k: p.grad.detach() for k, p in params.items()}, {k: v.detach() for k, v in out.items()}


def _module(bb, heads, mt, sd, **kw):
    from sleap_nn_amd.architectures.model import Model
    from sleap_nn_amd.training.module import TrainingModule

    m = Model("swint", bb, heads, mt)
    m.load_state_dict(sd, strict=True)
    kw.setdefault("stochastic_depth_prob", 0.0)
    return TrainingModule(m, DEV, loss_weights=[1.0], swint_training=True, **kw)


def _errors(got, ref):
    assert set(got) == set(ref), set(got) ^ set(ref)
    return {k: float((got[k].cpu() - r).abs().max()) / max(float(r.abs().max()), 1e-12) for k, r in ref.items()}


def _check(tm, loss, ref_loss, ref_grads):
    torch.cuda.synchronize()
    got = tm.named_grads()
    errs = _errors(got, ref_grads)
    worst = sorted(errs.items(), key=lambda kv: -kv[1])[:4]
    print("loss", float(loss[0]), ref_loss, "worst", worst)
    assert abs(float(loss[0]) - ref_loss) <= LOSS_RTOL * max(1.0, abs(ref_loss))
    bad = {k: v for k, v in errs.items() if v > GRAD_BAR}
    assert not bad, sorted(bad.items(), key=lambda kv: -kv[1])[:8]
    return got


def _case(bb, img, seed, mt=MT, n_parts=3, sd=None, scales=None, ref_step=_ref_step, **module_kw):
    heads = _heads(n_parts)
    sd = R.init_state_swint(bb, heads, mt, seed=seed) if sd is None else sd
    with torch.no_grad():
        shapes = {k: v.shape for k, v in R.model_forward(sd, bb, heads, mt, img).items()}
    g = torch.Generator().manual_seed(seed + 100)
    targets = {k: torch.rand(s, generator=g) * 0.5 for k, s in shapes.items()}
    ref_loss, ref_grads, _ = ref_step(sd, bb, heads, mt, img, targets)
    tm = _module(bb, heads, mt, sd, **module_kw)
    if scales is not None:
        tm.set_branch_scales(scales)
    loss = tm.forward_backward(img.to(DEV), {k: v.to(DEV) for k, v in targets.items()})
    got = _check(tm, loss, ref_loss, ref_grads)
    return tm, sd, heads, targets, ref_grads, got


def test_window7_padding_both_axes_shift_single_window_and_route():
    """64x96, window 7: stage maps 32x48, 16x24, 8x12, 4x6 -> padding on both axes under a shift, two 32-token tiles, a single window whose shift is forced off.
    Every float parameter receives a gradient; the attention-backward kernel is reported once per block; the arena's bucket split stays a parameter boundary."""
    from sleap_nn_amd import _lib as L

    bb = _bb()
    tm, sd, _heads_, _t, ref_grads, got = _case(bb, _img((2, 1, 64, 96), 11), seed=7, n_parts=5)
    assert all(float(g.abs().max()) > 0 for g in ref_grads.values())
    codes = tm.model.last_backward_kernels()
    assert codes.count(L.SWIN_KV_WINDOW_ATTN_BWD) == sum(SMALL["depths"])
    assert all(c == L.SWIN_KV_WINDOW_ATTN_BWD for c, o in zip(codes, tm.model.ops) if o.kind == L.OP_WINDOW_ATTN)
    split = int(L.check(L.lib().ph_model_grad_bucket_split(tm.model._handle)))
    bounds, o = set(), 0
    for k in tm.model.param_keys():
        bounds.add(o)
        o += int(torch.tensor(tm.model.param_shapes[k]).prod())
    assert 0 < split < o and split in bounds
    assert float(tm.padded_token_vector(2, 64, 96).abs().max()) > 0  # the first block's 32x48 map is padded to 35x49


def test_window4_one_tile_half_dead():
    _case(_bb(window_size=4), _img((2, 1, 64, 96), 12), seed=8)


def test_window8_two_full_tiles_no_padding_pad_vector_is_zero():
    """64x64, window 8: the first block's 32x32 map needs no padding, so the padded-token vector it leaves is exactly zero."""
    tm, *_ = _case(_bb(window_size=8), _img((2, 1, 64, 64), 13), seed=9)
    v = tm.padded_token_vector(2, 64, 64)
    assert v.numel() == 3 * SMALL["embed"] and float(v.abs().max()) == 0.0


def test_mixed_shift_rows_off_columns_on():
    """64x192: the last stage is 4x12 -> pH = 7 turns the row shift off, pW = 14 keeps the column shift on."""
    _case(_bb(), _img((2, 1, 64, 192), 14), seed=10)


def _window_attention_pad_detached(x, qkv_w, qkv_b, proj_w, proj_b, table, ws, heads, shift, index=None):
    """swin_ref.window_attention with the padded tokens' q, k, v cut off from qkv.bias's gradient (same values)."""
    B, H, W, Cc = x.shape
    pr, pb = (ws - W % ws) % ws, (ws - H % ws) % ws
    real = F.pad(x.new_ones((B, H, W, 1)), (0, 0, 0, pr, 0, pb))
    x = F.pad(x, (0, 0, 0, pr, 0, pb))
    _, pH, pW, _ = x.shape
    sh = [0 if ws >= pH else shift, 0 if ws >= pW else shift]
    if sum(sh) > 0:
        x = torch.roll(x, shifts=(-sh[0], -sh[1]), dims=(1, 2))
        real = torch.roll(real, shifts=(-sh[0], -sh[1]), dims=(1, 2))
    nW = (pH // ws) * (pW // ws)
    N = ws * ws

    def windows(t):
        return t.view(B, pH // ws, ws, pW // ws, ws, t.shape[-1]).permute(0, 1, 3, 2, 4, 5).reshape(B * nW, N, t.shape[-1])

    x, real = windows(x), windows(real)
    qkv = F.linear(x, qkv_w, qkv_b) * real + F.linear(x, qkv_w, qkv_b.detach()) * (1 - real)
    qkv = qkv.reshape(x.size(0), N, 3, heads, Cc // heads).permute(2, 0, 3, 1, 4)
    q, k, v = qkv[0] * (Cc // heads) ** -0.5, qkv[1], qkv[2]
    attn = q.matmul(k.transpose(-2, -1))
    idx = R.rel_index(ws) if index is None else index
    attn = attn + table[idx].view(N, N, -1).permute(2, 0, 1).unsqueeze(0)
    if sum(sh) > 0:
        m = x.new_zeros((pH, pW))
        c = 0
        for h in ((0, -ws), (-ws, -sh[0]), (-sh[0], None)):
            for w in ((0, -ws), (-ws, -sh[1]), (-sh[1], None)):
                m[h[0]: h[1], w[0]: w[1]] = c
                c += 1
        m = m.view(pH // ws, ws, pW // ws, ws).permute(0, 2, 1, 3).reshape(nW, N)
        m = m.unsqueeze(1) - m.unsqueeze(2)
        m = m.masked_fill(m != 0, -100.0).masked_fill(m == 0, 0.0)
        attn = (attn.view(x.size(0) // nW, nW, heads, N, N) + m.unsqueeze(1).unsqueeze(0)).view(-1, heads, N, N)
    attn = F.softmax(attn, dim=-1)
    x = F.linear(attn.matmul(v).transpose(1, 2).reshape(x.size(0), N, Cc), proj_w, proj_b)
    x = x.view(B, pH // ws, pW // ws, ws, ws, Cc).permute(0, 1, 3, 2, 4, 5).reshape(B, pH, pW, Cc)
    if sum(sh) > 0:
        x = torch.roll(x, shifts=(sh[0], sh[1]), dims=(1, 2))
    return x[:, :H, :W, :].contiguous()


def test_padded_tokens_gradient_reaches_qkv_bias(monkeypatch):
    """qkv.bias = +-3 in a padded plain block and a padded shifted block (32x48 -> 35x49): its gradient meets the bar, and it is not the gradient that leaves
    the padded tokens' share out (the reference rerun with the padded tokens' q, k, v detached from the bias).  The image seed is one whose smallest decoder
    ReLU pre-activation is 1.3e-5 in the reference: seed 15 has one at 5e-7, inside the forward's error (6e-6 there), and the device then takes the other branch
    of that kink -- every gradient upstream of that decoder conv moves by ~1e-3 of scale with an exact forward (measured; not a property of the kernels)."""
    bb, heads = _bb(), _heads(3)
    img = _img((2, 1, 64, 96), 36)
    sd = R.init_state_swint(bb, heads, MT, seed=9)
    g = torch.Generator().manual_seed(13)
    keys = [f"backbone.enc.features.1.{j}.attn.qkv.bias" for j in (0, 1)]
    for key in keys:
        sd[key] = torch.sign(torch.randn(sd[key].shape, generator=g)) * 3.0
    _tm, _sd, _h, targets, ref_grads, got = _case(bb, img, seed=9, sd=sd)
    with torch.no_grad():  # the restatement computes what swin_ref computes
        x = torch.randn((2, 10, 12, 32), generator=g)
        args = (sd[keys[1].replace("qkv.bias", "qkv.weight")], sd[keys[1]], sd[keys[1].replace("qkv.bias", "proj.weight")], sd[keys[1].replace("qkv.bias", "proj.bias")],
                sd[keys[1].replace("qkv.bias", "relative_position_bias_table")], 7, 1, 3)
        assert torch.allclose(_window_attention_pad_detached(x, *args), R.window_attention(x, *args), atol=1e-6)
    monkeypatch.setattr(R, "window_attention", _window_attention_pad_detached)
    _loss, cut_grads, _ = _ref_step(sd, bb, heads, MT, img, targets)
    for key in keys:
        scale = float(ref_grads[key].abs().max())
        share = float((ref_grads[key] - cut_grads[key]).abs().max()) / scale
        off = float((got[key].cpu() - cut_grads[key]).abs().max()) / scale
        print(key, "padded share", share, "device vs cut", off)
        assert share > 10 * GRAD_BAR and off > 10 * GRAD_BAR, (key, share, off)


def test_many_windows_per_slice_crop0_invariant_and_bitwise_repeatable():
    """B = 16 at 64x96: 560 windows in the first stage, more than the attention backward has workgroups, so each walks several windows.  With every other
    crop's target set to its own prediction (their output gradients are exactly zero), B times the batch's gradients are crop 0's own, to the bar; two
    identical steps give bitwise identical gradients."""
    bb, heads = _bb(), _heads(3)
    B = 16
    img = _img((B, 1, 64, 96), 16)
    sd = R.init_state_swint(bb, heads, MT, seed=21)
    tm = _module(bb, heads, MT, sd)
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


def _scaled_block(scales):
    """swin_ref.swin_block with each residual branch multiplied per sample: rows 2k, 2k + 1 of ``scales`` for the k-th block called."""
    state = {"k": 0}

    def block(sd, n, x, ws, heads, shift, collect=None):
        Cc = x.shape[-1]
        sa, sm = (scales[2 * state["k"] + i].view(-1, 1, 1, 1) for i in (0, 1))
        state["k"] += 1
        y = F.layer_norm(x, (Cc,), sd[n + ".norm1.weight"], sd[n + ".norm1.bias"], R.EPS)
        x = x + sa * R.window_attention(y, sd[n + ".attn.qkv.weight"], sd[n + ".attn.qkv.bias"], sd[n + ".attn.proj.weight"], sd[n + ".attn.proj.bias"],
                                        sd[n + ".attn.relative_position_bias_table"], ws, heads, shift)
        y = F.layer_norm(x, (Cc,), sd[n + ".norm2.weight"], sd[n + ".norm2.bias"], R.EPS)
        y = F.linear(F.gelu(F.linear(y, sd[n + ".mlp.0.weight"], sd[n + ".mlp.0.bias"])), sd[n + ".mlp.3.weight"], sd[n + ".mlp.3.bias"])
        return x + sm * y

    return block


def test_explicit_branch_scales(monkeypatch):
    """Scales 0, 1 / (1 - p) and 1 against the scaled restatement of the block.  Block 2's MLP branch is dropped for both samples: its parameters' gradients
    are exactly zero; block 1's attention branch is dropped for sample 0 only: its parameters see sample 1 alone, as the reference does."""
    bb = _bb()
    n = 2 * sum(SMALL["depths"])
    scales = torch.ones((n, 2))
    scales[2] = torch.tensor([0.0, 1.0 / (1.0 - 0.1 / 7)])       # block 1, attention branch
    scales[3] = torch.tensor([1.0 / (1.0 - 0.1 / 7), 1.0])
    scales[5] = torch.tensor([0.0, 0.0])                         # block 2, MLP branch
    scales[9] = torch.tensor([1.25, 0.0])
    scales[14] = torch.tensor([0.0, 1.0 / 0.9])

    def ref_step(sd, bb_, heads, mt, img, targets):
        monkeypatch.setattr(R, "swin_block", _scaled_block(scales))
        try:
            return _ref_step(sd, bb_, heads, mt, img, targets)
        finally:
            monkeypatch.undo()

    tm, _sd, _h, _t, ref_grads, got = _case(bb, _img((2, 1, 64, 96), 17), seed=23, scales=scales, ref_step=ref_step)
    blk = "backbone.enc.features.3.0"  # block 2 = first block of stage 1
    for name in (".norm2.weight", ".norm2.bias", ".mlp.0.weight", ".mlp.0.bias", ".mlp.3.weight", ".mlp.3.bias"):
        assert float(ref_grads[blk + name].abs().max()) == 0.0
        assert float(got[blk + name].abs().max()) == 0.0, name
    assert tm._active_scales is None and tm._next_scales is None  # used once, cleared after the backward


def test_three_adam_steps_match_reference_optimizer():
    """Three steps against torch.optim.Adam driven by the reference gradients, stochastic depth off; the entry-wise movement bars of
    test_convnext_adam_steps_reduce_loss_and_match_reference_optimizer; the loss goes down.  The middle block works on a 2x2 map here, where one ReLU
    that takes the other branch of its kink moves a whole row of weight gradients: the image seed is one whose smallest pre-activation on the maps of at most
    4x6 pixels stays above 1.3e-5 in all three reference steps (seed 18 comes within 1.1e-5 and one middle-conv entry then moves 2.7 % instead of 2 %)."""
    bb, heads = _bb(), _heads(3)
    img = _img((2, 1, 64, 64), 30)
    tm, sd, heads, targets, _rg, _got = _case(bb, img, seed=29, wino4=False)
    # Where the reference's gradient of a decoder / middle conv weight entry is EXACTLY zero (dead ReLU channels: a third of those entries here), the Winograd-domain
    # weight-gradient kernel leaves ~1e-12 instead of 0, and Adam's m / (sqrt(v) + eps) turns that into 0.1 lr in the first step and 2.5 lr by the third (measured:
    # 0.86 of the possible movement, then a cascade).  The direct weight-gradient kernel keeps those zeros exact, as the reference does.
    tm.model.set_option("wgrad_wino", 0)
    floats = {k: v for k, v in sd.items() if v.is_floating_point()}
    opt_params = {k: torch.nn.Parameter(v.clone()) for k, v in floats.items()}
    opt = torch.optim.Adam(list(opt_params.values()), lr=1e-3)
    tm.lr = 1e-3
    batch = {"image": img.to(DEV), **{k: v.to(DEV) for k, v in targets.items()}}
    first = None
    tiny = {k: torch.zeros_like(v, dtype=torch.bool) for k, v in floats.items()}
    for _step in range(3):
        _, grads, _ = _ref_step({**sd, **{k: p.detach() for k, p in opt_params.items()}}, bb, heads, MT, img, targets)
        for k, p in opt_params.items():
            p.grad = grads[k]
            tiny[k] |= (grads[k].abs() < 1e-3 * grads[k].abs().max()) & (grads[k] != 0)
        opt.step()
        loss = tm.training_step(batch)
        first = float(loss[0]) if first is None else first
    torch.cuda.synchronize()
    got = tm.state_dict()
    over = {}
    for k, p in opt_params.items():
        d = (got[k].cpu() - p.detach()).abs()
        big = d[~tiny[k]]
        strict, loose = (float(big.max()) if big.numel() else 0.0) / 3e-3, float(d.max()) / 3e-3
        if strict > 0.02 or loose > 0.10:
            over[k] = (round(strict, 4), round(loose, 4))
    print("worst movement differences (share of 3 x lr; entries with a non-tiny gradient, all entries):", sorted(over.items(), key=lambda kv: -kv[1][1])[:12])
    assert float(loss[0]) < first
    assert not over, sorted(over.items(), key=lambda kv: -kv[1][1])[:8]
    assert sum(int(t.sum()) for t in tiny.values()) < 0.5 * sum(t.numel() for t in tiny.values())
    assert float(loss[0]) < first


def test_swin_tiny_backward_matches_autograd():
    """model_type "tiny" (96..768 channels over 3 / 6 / 12 / 24 heads, six blocks in stage 2), 64x96, B = 2, 13 nodes: the same bars."""
    bb = _bb(model_type="tiny", arch=None)
    tm, *_ = _case(bb, _img((2, 1, 64, 96), 19), seed=41, mt="centered_instance", n_parts=13)
    assert tm.params.numel() > 1 << 24


def test_eval_after_stochastic_training_step():
    """After a stochastic step and eval(): no scales remain set (a forward of another batch size runs), and the inference forward of the trained handle equals
    that of a fresh handle loaded from tm.state_dict()."""
    from sleap_nn_amd.architectures.model import Model

    bb, heads = _bb(), _heads(3)
    img = _img((2, 1, 64, 96), 20)
    sd = R.init_state_swint(bb, heads, MT, seed=31)
    tm = _module(bb, heads, MT, sd, stochastic_depth_prob=0.5, stochastic_depth_seed=3)
    with torch.no_grad():
        shape = R.model_forward(sd, bb, heads, MT, img)[HEAD].shape
    tgt = torch.rand(shape, generator=torch.Generator().manual_seed(1)).to(DEV) * 0.5
    loss = tm.training_step({"image": img.to(DEV), HEAD: tgt})
    torch.cuda.synchronize()
    assert torch.isfinite(loss).all()
    s = tm.last_branch_scales.cpu()
    assert s.shape == (16, 2) and bool((s[:2] == 1).all()) and bool((s == 0).any())  # block 0 is never dropped; p up to 0.5 drops something (seeded)
    assert tm._active_scales is None
    tm.model.eval()
    got = tm.model(img[:1].to(DEV))[HEAD].clone()  # batch 1: refused if the scales of the batch-2 step were still set
    fresh = Model("swint", bb, heads, MT)
    fresh.load_state_dict(tm.state_dict(), strict=True)
    want = fresh.to(DEV)(img[:1].to(DEV))[HEAD]
    torch.cuda.synchronize()
    assert torch.equal(got, want)


def test_refusals():
    from sleap_nn_amd import _lib as L
    from sleap_nn_amd.architectures.model import Model
    from sleap_nn_amd.training.module import TrainingModule

    bb, heads = _bb(), _heads(3)
    sd = R.init_state_swint(bb, heads, MT, seed=33)
    m = Model("swint", bb, heads, MT)
    m.load_state_dict(sd, strict=True)
    with pytest.raises(NotImplementedError, match="allow_swint"):
        m.train()
    with pytest.raises(NotImplementedError, match="swint_training"):
        TrainingModule(m, DEV, loss_weights=[1.0])
    tm = TrainingModule(m, DEV, loss_weights=[1.0], swint_training=True)
    n = tm.model.residual_branches()
    assert n == 2 * sum(SMALL["depths"])
    scales = torch.ones((n + 1, 2), device=DEV)
    lib = L.lib()
    assert lib.ph_model_set_branch_scales(tm.model._handle, C.c_void_p(scales.data_ptr()), n + 1, 2) < 0
    assert b"residual" in lib.ph_last_error()
    assert lib.ph_model_set_branch_scales(tm.model._handle, C.c_void_p(scales.data_ptr()), n, 2) == 0
    with pytest.raises(L.PosehipError):  # a forward of another batch size while scales are set
        tm.model.forward(_img((1, 1, 64, 96), 1).to(DEV))
    assert lib.ph_model_set_branch_scales(tm.model._handle, None, 0, 0) == 0
    with pytest.raises(ValueError):
        tm.set_branch_scales(scales)
        tm.forward_backward(_img((2, 1, 64, 96), 1).to(DEV), {HEAD: torch.zeros((2, 3, 32, 48))})
