"""GPU parity of the Swin Transformer encoder-decoder path (inference, exact fp32) against tests/swin_ref.py.

The bar is that of tests/test_gpu_convnext.py: max error <= 1e-4 of max(1, scale), per labelled block (read_activation) and on the head outputs.  swin_ref
restates torchvision's public definition (tests/test_swint_cpu.py compares it with an independent implementation; torchvision itself is not installed).
Weights as ``init_state_convnext(randomize_affine=True)`` draws them, the relative-position bias table N(0, 0.5) so that the bias matters.
"""
import hashlib

import numpy as np
import pytest
import torch

from oracle import cpu_ref as O
from tests import swin_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ATOL = 1e-4
SMALL = {"embed": 32, "depths": [2, 2, 2, 2], "num_heads": [1, 2, 4, 8]}


def _bb(**kw):
    bb = {"model_type": None, "arch": SMALL, "in_channels": 1, "patch_size": 4, "window_size": 7, "kernel_size": 3, "filters_rate": 2, "convs_per_block": 2,
          "up_interpolate": True, "stem_patch_stride": 2, "output_stride": 2, "max_stride": 32, "pre_trained_weights": None}
    bb.update(kw)
    return bb


def _heads(n, stride=2):
    return {"confmaps": {"part_names": [str(i) for i in range(n)], "sigma": 2.5, "output_stride": stride}}


def _model(bb, heads, mt, sd, keep=False):
    from sleap_nn_amd.architectures.model import Model

    m = Model("swint", bb, heads, mt)
    m.load_state_dict(sd, strict=True)
    m.to(DEV).set_keep_activations(keep)
    return m


def _err(got, want):
    return (got - want).abs().max().item() / max(1.0, want.abs().max().item())


def _run(bb, heads, mt, img, seed=7, check_blocks=True, sd=None):
    """Forward on the device against swin_ref: per labelled block (keep-activations plan) and on the heads -> (model, state, reference outputs, device outputs)."""
    sd = R.init_state_swint(bb, heads, mt, seed=seed) if sd is None else sd
    collect = {}
    ref = R.model_forward(sd, bb, heads, mt, img, collect=collect)
    m = _model(bb, heads, mt, sd, keep=check_blocks)
    out = m(img.to(DEV))
    torch.cuda.synchronize()
    if check_blocks:
        checked = 0
        for name, t in collect.items():
            if name not in m.backbone.labels:
                continue
            got = m.read_activation(name, t.shape[0], t.shape[-2:]).cpu()
            e = _err(got, t)
            print(f"{name}: {e:.3g} (scale {t.abs().max().item():.3g})")
            assert e <= ATOL, (name, e, t.abs().max().item())
            checked += 1
        assert checked >= 4 * sum(R.arch_of(bb)["depths"]) // 2
    for k, t in ref.items():
        got = out[k].cpu()
        assert got.shape == t.shape
        e = _err(got, t)
        print(f"{k}: {e:.3g}")
        assert e <= ATOL, (k, e)
    return m, sd, ref, out


def _check_plan(m, where):
    from tests.test_gpu_plan_hazards import _check_plan as check

    return check(m, where)


def test_small_arch_padding_both_axes_shift_and_single_window():
    """Stage maps 32x48, 16x24, 8x12, 4x6 -> padded 35x49, 21x28, 14x14, 7x7: padding in both axes under a shift, and a single window whose shift is forced off.
    The plan that recycles slots gives the same maps, passes the no-overlap / liveness invariant of tests/test_gpu_plan_hazards.py (the block input stays live
    across both residual adds), and ``set_precision`` leaves the program exact."""
    from sleap_nn_amd import _lib as L

    bb, heads = _bb(), _heads(5)
    g = torch.Generator().manual_seed(11)
    img = torch.randint(0, 256, (2, 1, 64, 96), dtype=torch.uint8, generator=g)
    m, sd, ref, out = _run(bb, heads, "single_instance", img)
    assert list(m.last_kernels()).count(L.SWIN_KV_WINDOW_ATTN) == 8
    r = _model(bb, heads, "single_instance", sd)
    got = r(img.to(DEV))["SingleInstanceConfmapsHead"].clone()
    torch.cuda.synchronize()
    assert _err(got.cpu(), ref["SingleInstanceConfmapsHead"]) <= ATOL
    _check_plan(r, "swint small")
    # every residual Linear was handed its block input as a source while the launches between them ran
    rows = r.last_ranges()
    for p, o in enumerate(r.ops):
        if o.kind == L.OP_LINEAR and o.flags & L.FLAG_RESIDUAL:
            assert any(op == p and not is_dst and slot == o.src1 for op, _ln, is_dst, slot, _o, _n in rows), p
    for prec in ("split", "fp16"):
        r.set_precision(prec)
        again = r(img.to(DEV))["SingleInstanceConfmapsHead"]
        torch.cuda.synchronize()
        assert torch.equal(again, got), prec
        assert L.SWIN_KV_WINDOW_ATTN in r.last_kernels()


def test_mixed_shift_rows_off_columns_on():
    """64x192: the last stage is 4x12 -> pH = 7 turns the row shift off, pW = 14 keeps the column shift on."""
    bb, heads = _bb(), _heads(3)
    g = torch.Generator().manual_seed(12)
    img = torch.randint(0, 256, (2, 1, 64, 192), dtype=torch.uint8, generator=g)
    _run(bb, heads, "single_instance", img, seed=8)


def test_padded_tokens_take_part_as_keys():
    """A padded token's q, k, v are exactly qkv.bias and nothing but the band rule masks it: with a large bias (+-3) in a block whose map is padded in both axes
    the result still meets the bar, and it differs from the run with that bias zeroed."""
    bb, heads = _bb(), _heads(3)
    g = torch.Generator().manual_seed(13)
    img = torch.randint(0, 256, (2, 1, 64, 96), dtype=torch.uint8, generator=g)
    sd = R.init_state_swint(bb, heads, "single_instance", seed=9)
    outs = []
    for scale in (3.0, 0.0):
        for blk in ("backbone.enc.features.1.0", "backbone.enc.features.1.1"):  # 32x48 -> 35x49, plain and shifted
            key = blk + ".attn.qkv.bias"
            sd[key] = torch.sign(torch.randn(sd[key].shape, generator=g)) * scale
        _m, _sd, _ref, out = _run(bb, heads, "single_instance", img, sd=sd)
        outs.append(out["SingleInstanceConfmapsHead"].cpu())
    assert (outs[0] - outs[1]).abs().max().item() > 100 * ATOL


@pytest.mark.parametrize("window", [4, 8])
def test_window_4_and_8(window):
    """N = 16 (one 32-token tile, half of it dead) and N = 64 (two full tiles)."""
    bb, heads = _bb(window_size=window), _heads(3)
    g = torch.Generator().manual_seed(14)
    img = torch.randint(0, 256, (1, 1, 64, 64), dtype=torch.uint8, generator=g)
    _run(bb, heads, "single_instance", img, seed=10 + window)


def test_swin_tiny_centered_instance_rgb_float():
    """Swin-tiny: 96..768 channels over 3 / 6 / 12 / 24 heads, the 1536-channel merge norm, a parameter arena above 2^24; plan invariant on the recycling plan."""
    bb = _bb(model_type="tiny", arch=None, in_channels=3)
    heads = _heads(13)
    g = torch.Generator().manual_seed(3)
    img = torch.rand((1, 3, 64, 64), generator=g)
    m, _sd, _ref, _out = _run(bb, heads, "centered_instance", img, check_blocks=False)
    assert m.num_parameters() > 1 << 24
    _check_plan(m, "swint tiny")


def test_more_than_one_round_of_workgroups_is_batch_invariant():
    """Batch 4 at 128x128: 400 windows at stage 0.  window_attn_kernel is not persistent (grid = ceil(windows * heads / 4) workgroups of four waves, read from
    launch_window_attn), so 'rounds' are the hardware's: 100 workgroups per frame at stage 0, 400 in the launch.  Frame 2 of the batch equals the same frame run alone, bit for bit."""
    bb, heads = _bb(), _heads(3)
    g = torch.Generator().manual_seed(15)
    img = torch.randint(0, 256, (4, 1, 128, 128), dtype=torch.uint8, generator=g)
    m, _sd, _ref, _out = _run(bb, heads, "single_instance", img, seed=21, check_blocks=False)
    m.set_option("conv_wino4", 3)  # (the decoder's 3x3 kernel choice depends on the tile count, i.e. on the batch: one choice for the bitwise comparison, as in tests/test_gpu_convnext.py)
    m.set_option("conv_splitk", 0)
    m.set_option("conv_smallmap", 0)
    o4 = m(img.to(DEV))["SingleInstanceConfmapsHead"][2:3].clone()
    o1 = m(img[2:3].to(DEV))["SingleInstanceConfmapsHead"]
    torch.cuda.synchronize()
    assert torch.equal(o4, o1)


# sha256 of the head output of the ConvNeXt forward below at the commit before the Swin ops (and their LayerNorm eps flag) existed
CONVNEXT_SHA256 = "8957d1583138f1bd46b914cc4a425da6a792c02872fbc442e7b4995f365d6e99"


def test_convnext_forward_is_bitwise_what_it_was():
    """The per-op LayerNorm eps did not leak: a ConvNeXt program ([16, 32, 64, 128] x [1, 2, 1, 1], 64x96) reproduces its earlier output bit for bit."""
    from sleap_nn_amd.architectures.model import Model

    bb = {"model_type": None, "arch": {"depths": [1, 2, 1, 1], "channels": [16, 32, 64, 128]}, "in_channels": 1, "kernel_size": 3, "filters_rate": 2, "convs_per_block": 2,
          "up_interpolate": True, "stem_patch_kernel": 4, "stem_patch_stride": 2, "output_stride": 2, "max_stride": 32}
    heads = _heads(5)
    g = torch.Generator().manual_seed(11)
    img = torch.randint(0, 256, (2, 1, 64, 96), dtype=torch.uint8, generator=g)
    sd = O.init_state_convnext(bb, heads, "single_instance", seed=7, head_scale=1.0, layer_scale=0.5, randomize_affine=True)
    m = Model("convnext", bb, heads, "single_instance")
    m.load_state_dict(sd, strict=True)
    out = m.to(DEV)(img.to(DEV))["SingleInstanceConfmapsHead"].cpu().contiguous()
    assert hashlib.sha256(out.numpy().tobytes()).hexdigest() == CONVNEXT_SHA256


def test_predictor_loads_a_swint_run_directory(tmp_path):
    """training_config.yaml with a swint backbone block and a bottom-up head + best.ckpt with the Lightning prefix and the index buffers -> Predictor.from_model_paths
    -> peaks and grouping equal to the oracle's bottom-up post-process on swin_ref's maps."""
    import yaml

    from sleap_nn_amd.inference.predictor import Predictor

    names = [str(i) for i in range(4)]
    edges = [[names[i], names[i + 1]] for i in range(3)]
    bb = _bb(pre_trained_weights="Swin_T_Weights")  # ignored at load: the checkpoint holds the weights
    heads = {"confmaps": {"part_names": names, "sigma": 2.5, "output_stride": 2, "loss_weight": 1.0},
             "pafs": {"edges": edges, "sigma": 15.0, "output_stride": 4, "loss_weight": 1.0}}
    sd = R.init_state_swint(bb, heads, "bottomup", seed=31)
    cfg = {"data_config": {"preprocessing": {"scale": 1.0},
                           "skeletons": [{"name": "s", "nodes": [{"name": n} for n in names], "edges": [{"source": {"name": a}, "destination": {"name": b}} for a, b in edges]}]},
           "model_config": {"backbone_config": {"unet": None, "convnext": None, "swint": bb}, "head_configs": {"bottomup": heads}}}
    with open(tmp_path / "training_config.yaml", "w") as f:
        yaml.safe_dump(cfg, f)
    torch.save({"state_dict": {"model." + k: v for k, v in sd.items()}}, tmp_path / "best.ckpt")
    g = torch.Generator().manual_seed(17)
    img = torch.randint(0, 256, (2, 1, 64, 96), dtype=torch.uint8, generator=g)
    ref = R.model_forward(sd, bb, heads, "bottomup", img)
    cms, pafs = ref["MultiInstanceConfmapsHead"], ref["PartAffinityFieldsHead"]
    thr = float(cms.mean() + 2 * cms.std())
    rk, rv, _rs = O.bottomup_postprocess(cms, pafs, O.PAFScorerRef(names, [tuple(e) for e in edges], 4), 2, peak_threshold=thr)
    assert int((~np.isnan(rk[..., 0])).sum()) >= 3, "the frames must yield a few peaks"
    p = Predictor.from_model_paths([str(tmp_path)], device=DEV, batch_size=2, peak_threshold=thr)
    outs = p.predict(img.numpy())
    assert len(outs) == 1
    k = outs[0].pred_keypoints.cpu().numpy()
    assert k.shape == rk.shape, (k.shape, rk.shape)
    assert np.array_equal(np.isnan(k), np.isnan(rk))
    assert np.allclose(k, rk, atol=1e-3, equal_nan=True)
    scale = max(1.0, float(cms.abs().max()))
    assert np.allclose(outs[0].pred_peak_values.cpu().numpy(), rv, atol=ATOL * scale, equal_nan=True)
