"""Training the ``pretrained`` (ConvNeXtV2) backbone, the parts that need no GPU: the GRN backward formula that csrc/convnextv2_train_kernels.hip implements against
torch autograd over ``convnextv2_ref.grn`` in float64, the opt-in keywords and the refusals that name them, the optimizer's ranges of the flat parameter arena
(unread and frozen parameters left out), and the refusal of a non-zero ``drop_path_rate``."""
import inspect
import json
import os

import pytest
import torch

from tests import convnextv2_ref as R
from tests.test_pretrained_cpu import PARTS, RUN_DIR, bb_of, heads_of

STEM_NORM = ("backbone.enc.hidden_states_norms.stem.weight", "backbone.enc.hidden_states_norms.stem.bias")


def grn_backward(x, w, g, c_true=None):
    """The kernels' formula.  ``x``, ``g``: (B, H, W, C); ``w``: (C,).  -> (dx, dw, dbeta)."""
    C = x.shape[-1] if c_true is None else c_true
    s = (x * x).sum(dim=(1, 2))                      # (B, C)
    G = s.sqrt()
    D = G.mean(dim=-1, keepdim=True) + 1e-6          # (B, 1)
    N = G / D
    T = (g * x).sum(dim=(1, 2))                      # (B, C)
    dbeta = g.sum(dim=(0, 1, 2))
    dw = (T * N).sum(dim=0)
    dN = w * T
    dG = dN / D - (dN * G).sum(dim=-1, keepdim=True) / (C * D * D)
    K = torch.where(G > 0, dG / torch.where(G > 0, G, torch.ones_like(G)), torch.zeros_like(G))
    dx = g * (1 + w * N)[:, None, None, :] + x * K[:, None, None, :]
    return dx, dw, dbeta


@pytest.mark.parametrize("dtype,bar", [(torch.float64, 1e-13), (torch.float32, 1e-6)])
def test_grn_backward_formula_matches_autograd(dtype, bar):
    """Against autograd over convnextv2_ref.grn, with a channel that is exactly zero for one sample (3) and one that is zero for all (5): autograd's gradient is
    finite there and K = 0 reproduces it."""
    gen = torch.Generator().manual_seed(3)
    B, H, W, C = 3, 5, 7, 12
    x = torch.randn(B, H, W, C, generator=gen, dtype=torch.float64)
    x[1] *= 0.2
    x[0, :, :, 3] = 0
    x[:, :, :, 5] = 0
    w = torch.randn(C, generator=gen, dtype=torch.float64)
    beta = torch.randn(C, generator=gen, dtype=torch.float64)
    g = torch.randn(B, H, W, C, generator=gen, dtype=torch.float64)
    x, w, beta, g = (t.to(dtype) for t in (x, w, beta, g))
    xr, wr, br = x.clone().requires_grad_(True), w.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    R.grn(xr, wr.view(1, 1, 1, C), br.view(1, 1, 1, C)).backward(g)
    assert torch.isfinite(xr.grad).all()
    dx, dw, dbeta = grn_backward(x, w, g)
    for name, got, want in (("dx", dx, xr.grad), ("dw", dw, wr.grad), ("dbeta", dbeta, br.grad)):
        err = float((got - want).abs().max()) / float(want.abs().max())
        print(name, err)
        assert torch.isfinite(got).all() and err <= bar, (name, err)
    assert float(dx[0, :, :, 3].abs().max()) > 0 and torch.equal(dx[:, :, :, 5], g[:, :, :, 5])  # a zero channel passes g through: 1 + w N = 1, x K = 0


def _model(freeze=False, model_name=None):
    from sleap_nn_amd.architectures.model import Model

    bb = dict(bb_of("A", model_name or os.path.join(RUN_DIR, "hf_config")), freeze=freeze)
    return Model("pretrained", bb, heads_of("A"), "single_instance")


def test_opt_in_keywords_and_refusals_name_them():
    from sleap_nn_amd.architectures.model import Model
    from sleap_nn_amd.training.module import TrainingModule
    from sleap_nn_amd.training.segmentation import SegmentationTrainingModule

    assert "allow_pretrained" in inspect.signature(Model.train).parameters
    sig = inspect.signature(TrainingModule.__init__).parameters
    assert "pretrained_training" in sig and "freeze_encoder" in sig
    assert sig["pretrained_training"].default is False and sig["freeze_encoder"].default is None
    assert any(p.kind is inspect.Parameter.VAR_KEYWORD for p in inspect.signature(SegmentationTrainingModule.__init__).parameters.values())  # passes it through
    m = _model()
    with pytest.raises(NotImplementedError, match="pretrained.*allow_pretrained"):
        m.train()
    with pytest.raises(NotImplementedError, match="pretrained.*pretrained_training"):
        TrainingModule(m)
    from sleap_nn_amd import _lib as L

    assert all(o.flags & L.FLAG_NO_TRAIN for o in m.unfused_ops if o.kind in (L.OP_GRN, L.OP_PATCH_STEM))
    assert m.train(True, allow_pretrained=True).ops is m.unfused_ops and m._options["pretrained_train"] == 1.0
    assert all(o.flags & L.FLAG_NO_TRAIN for o in m.unfused_ops if o.kind in (L.OP_GRN, L.OP_PATCH_STEM))  # the flags stay; the handle option lifts the refusal
    assert m.eval().ops is m.fused_ops
    unet = Model("unet", {"in_channels": 1, "kernel_size": 3, "filters": 8, "filters_rate": 2, "max_stride": 16, "stem_stride": None, "middle_block": True, "up_interpolate": True,
                          "stacks": 1, "convs_per_block": 2, "output_stride": 2}, {"confmaps": {"part_names": PARTS, "sigma": 2.5, "output_stride": 2}}, "single_instance")
    with pytest.raises(ValueError, match="freeze_encoder"):
        TrainingModule(unet, freeze_encoder=True)


def _ranges_complement(m, ranges):
    """Keys of the parameters outside ``ranges``; asserts that the ranges are sorted, disjoint, non-adjacent and on parameter boundaries."""
    bounds, spans, o = set(), {}, 0
    for k in m.param_keys():
        n = int(torch.tensor(m.param_shapes[k]).prod())
        spans[k] = (o, o + n)
        bounds.add(o)
        o += n
    bounds.add(o)
    assert o == m.num_parameters()
    prev = -1
    for lo, hi in ranges:
        assert prev < lo < hi <= o and lo in bounds and hi in bounds, (lo, hi)
        prev = hi
    inside = lambda a, b: any(lo <= a and b <= hi for lo, hi in ranges)  # noqa: E731
    touched = lambda a, b: any(lo < b and a < hi for lo, hi in ranges)  # noqa: E731
    out = set()
    for k, (a, b) in spans.items():
        assert inside(a, b) or not touched(a, b), k
        if not inside(a, b):
            out.add(k)
    return out


def test_trainable_ranges_of_the_arena():
    """Unfrozen: everything but the two stem-norm tensors, which no op reads.  Frozen (by the config or by the override): everything but ``backbone.enc.*``."""
    m = _model()
    assert _ranges_complement(m, m.trainable_ranges()) == set(STEM_NORM)
    assert _ranges_complement(m, m.trainable_ranges(False)) == set(STEM_NORM)
    enc = {k for k in m.param_keys() if k.startswith("backbone.enc.")}
    assert set(STEM_NORM) < enc and len(enc) < len(m.param_keys())
    assert _ranges_complement(m, m.trainable_ranges(True)) == enc
    fz = _model(freeze=True)
    assert fz.backbone.freeze is True
    assert _ranges_complement(fz, fz.trainable_ranges()) == enc and _ranges_complement(fz, fz.trainable_ranges(False)) == set(STEM_NORM)
    assert len(fz.trainable_ranges()) == 1  # decoder and heads lie behind the encoder in one piece
    # the frozen prefix of the backward sweep: every op with an encoder parameter, and the parameter-less GELUs between them; the decoder starts right behind
    n = m.backbone.encoder_ops()
    ops = m.unfused_ops
    assert all((o.weight or "backbone.enc.").startswith("backbone.enc.") for o in ops[:n]) and not any((o.weight or "").startswith("backbone.enc.") for o in ops[n:])
    assert ops[n - 1].weight == "backbone.enc.hidden_states_norms.stage4.weight" and ops[n].label.startswith("backbone.dec.")
    # a model without unread parameters: one range, the whole arena
    from sleap_nn_amd.architectures.model import Model

    unet = Model("unet", {"in_channels": 1, "kernel_size": 3, "filters": 8, "filters_rate": 2, "max_stride": 16, "stem_stride": None, "middle_block": True, "up_interpolate": True,
                          "stacks": 1, "convs_per_block": 2, "output_stride": 2}, {"confmaps": {"part_names": PARTS, "sigma": 2.5, "output_stride": 2}}, "single_instance")
    assert unet.trainable_ranges() == [(0, unet.num_parameters())]


def test_nonzero_drop_path_rate_is_refused_by_name(tmp_path):
    from sleap_nn_amd.architectures import pretrained as P
    from sleap_nn_amd.training.module import TrainingModule

    d = tmp_path / "hf_dp"
    d.mkdir()
    cfg = {"model_type": "convnextv2", "depths": [1, 1, 2, 1], "hidden_sizes": [16, 32, 48, 64], "patch_size": 4, "num_channels": 3, "hidden_act": "gelu", "drop_path_rate": 0.1}
    with open(d / "config.json", "w") as f:
        json.dump(cfg, f)
    assert P.resolve_architecture(str(d))["drop_path_rate"] == 0.1
    assert P.resolve_architecture(os.path.join(RUN_DIR, "hf_config"))["drop_path_rate"] == 0.0 and P.resolve_architecture("facebook/convnextv2-nano-22k-224")["drop_path_rate"] == 0.0
    m = _model(model_name=str(d))
    assert m.backbone.drop_path_rate == 0.1
    m.eval()  # inference ignores it
    with pytest.raises(NotImplementedError, match="drop_path_rate"):
        m.train(True, allow_pretrained=True)
    with pytest.raises(NotImplementedError, match="drop_path_rate"):
        TrainingModule(m, pretrained_training=True)
    with pytest.raises(NotImplementedError, match="allow_pretrained"):  # the bare call still names the keyword first
        m.train()
