"""GPU parity of the segmentation training path: the BCE + Dice and masked smooth-L1 kernels against a float64 evaluation of the reference
formulas, the mask-target kernels against the reference's recorded results and the CPU form, and the training step of both model types against the
reference's own ``training_step`` (tests/golden/seg_training.npz) and against an independent torch-autograd restatement.

Bars (the project's own): loss rtol 1e-5 and gradients within 1e-4 of the tensor's scale for the loss kernels (tests/test_gpu_training.py), against
float64; foreground, weight, offsets and centroids equal, heat map atol 2e-6; step losses rtol 2e-5 and parameter gradients within 2e-4 of each
tensor's scale (the bars of test_multiclass_topdown_training_matches_autograd for its non-MSE head)."""
import json

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import cpu_ref as O
from tests import _golden as G

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
Z = G.load("seg_training.npz")
TINY = G.load("unet_tiny_seg.npz")
LOSS_NAMES = json.loads(str(Z["losses/names"]))
TARGET_NAMES = json.loads(str(Z["targets/names"]))
CMS_ATOL = 1e-4  # tests/test_gpu_segmentation.py: the tolerance of unet_tiny_seg.npz's out/


# ---- loss kernels --------------------------------------------------------------------------------------------------------------------------

def bce_dice_ref(z, t, bw, dw, smooth, pw):
    """The reference formula (training/losses.py:64-105) on tensors of any float dtype -> (loss, d loss / d z)."""
    z = z.clone().requires_grad_(True)
    bce = F.binary_cross_entropy_with_logits(z, t, reduction="mean", pos_weight=None if pw is None else torch.as_tensor(pw, dtype=z.dtype))
    p = torch.sigmoid(z)
    inter = (p * t).sum(dim=(2, 3))
    union = p.sum(dim=(2, 3)) + t.sum(dim=(2, 3))
    loss = bw * bce + dw * (1.0 - ((2.0 * inter + smooth) / (union + smooth)).mean())
    (g,) = torch.autograd.grad(loss, z)
    return loss.detach(), g


def sl1_ref(p, y, m):
    p = p.clone().requires_grad_(True)
    me = m.expand_as(p)
    n = me.sum()
    if n == 0:
        return torch.zeros((), dtype=p.dtype), torch.zeros_like(p)
    loss = F.smooth_l1_loss(p * me, y * me, reduction="sum") / n
    (g,) = torch.autograd.grad(loss, p)
    return loss.detach(), g


def check_against_f64(tag, loss, grad, loss64, grad64, loss32, grad32):
    scale = max(float(grad64.abs().max()), 1e-30)
    e_loss = abs(float(loss) - float(loss64)) / max(abs(float(loss64)), 1e-30)
    e_grad = float((grad.double() - grad64).abs().max()) / scale
    c_loss = abs(float(loss32) - float(loss64)) / max(abs(float(loss64)), 1e-30)
    c_grad = float((grad32.double() - grad64).abs().max()) / scale
    print(f"{tag}: device vs float64: loss {e_loss:.2e}, grad {e_grad:.2e} of scale; torch CPU fp32 vs float64: loss {c_loss:.2e}, grad {c_grad:.2e}")
    assert not torch.isnan(grad).any()
    assert e_loss <= 1e-5, (tag, float(loss), float(loss64))
    assert e_grad <= 1e-4, (tag, e_grad, scale)


def bce_dice_inputs(B, h, w, target):
    g = torch.Generator().manual_seed(1000 * B + 10 * h + w)
    z = torch.randn((B, 1, h, w), generator=g) * 3.0
    t = (torch.rand((B, 1, h, w), generator=g) < 0.4).float() if target == "random" else torch.full((B, 1, h, w), 1.0 if target == "ones" else 0.0)
    if h * w >= 10:  # 0, +-30, +-80 against both target values (the all-zero / all-one targets keep theirs)
        zf, tf = z[0, 0].view(-1), t[0, 0].view(-1)
        for k, v in enumerate([0.0, 30.0, -30.0, 80.0, -80.0]):
            zf[2 * k], zf[2 * k + 1] = v, v
            if target == "random":
                tf[2 * k], tf[2 * k + 1] = 0.0, 1.0
    return z, t


@pytest.mark.parametrize("shape", [(1, 1, 1), (3, 5, 7), (2, 130, 131)])
def test_bce_dice_kernel_matches_float64(shape):
    from sleap_nn_amd.training.losses import compute_bce_dice_loss, compute_bce_dice_loss_with_grad

    B, h, w = shape
    for target in ("random", "zeros", "ones"):
        z, t = bce_dice_inputs(B, h, w, target)
        for pw in (None, 3.0):
            for bw, dw in ((0.5, 0.5), (1.0, 0.25)):
                l64, g64 = bce_dice_ref(z.double(), t.double(), bw, dw, 1.0, pw)
                l32, g32 = bce_dice_ref(z, t, bw, dw, 1.0, pw)
                loss, grad = compute_bce_dice_loss_with_grad(z.to(DEV), t.to(DEV), bce_weight=bw, dice_weight=dw, smooth=1.0, pos_weight=pw)
                check_against_f64(f"bce_dice {shape} {target} pw={pw} w=({bw},{dw})", loss.cpu(), grad.cpu(), l64, g64, l32, g32)
                loss2, grad2 = compute_bce_dice_loss_with_grad(z.to(DEV), t.to(DEV), bce_weight=bw, dice_weight=dw, smooth=1.0, pos_weight=pw)
                assert torch.equal(loss, loss2) and torch.equal(grad, grad2)  # a second launch is bitwise identical
                assert torch.equal(compute_bce_dice_loss(z.to(DEV), t.to(DEV), bw, dw, 1.0, pw), loss)
    # loss_weight scales the gradient only
    z, t = bce_dice_inputs(B, h, w, "random")
    l1, g1 = compute_bce_dice_loss_with_grad(z.to(DEV), t.to(DEV))
    l2, g2 = compute_bce_dice_loss_with_grad(z.to(DEV), t.to(DEV), loss_weight=0.25)
    assert torch.equal(l1, l2) and torch.allclose(g2, 0.25 * g1, rtol=1e-6, atol=0)


def sl1_inputs(B, h, w, mask):
    g = torch.Generator().manual_seed(7 * B + h + w)
    p = torch.randn((B, 2, h, w), generator=g) * 1.5
    y = torch.randn((B, 2, h, w), generator=g) * 1.5
    pf, yf = p.view(-1), y.view(-1)
    for k, (a, b) in enumerate(((0.75, -0.25), (-0.5, 0.5), (2.5, 1.5 - 1e-3), (-0.25, 0.75 + 1e-3), (0.5, 0.25), (3.0, -4.0))):  # exactly +-1, both sides of 1
        pf[k], yf[k] = a, b
    m = torch.zeros((B, 1, h, w))
    if mask == "random":
        m = (torch.rand((B, 1, h, w), generator=g) < 0.6).float()
        m.view(-1)[:6] = 1.0
    elif mask == "one_pixel":
        m[B - 1, 0, h // 2, w // 3] = 1.0
    return p, y, m


@pytest.mark.parametrize("shape", [(2, 6, 9), (2, 130, 131)])
@pytest.mark.parametrize("mask", ["random", "empty", "one_pixel"])
def test_masked_smooth_l1_kernel_matches_float64(shape, mask):
    from sleap_nn_amd.training.losses import compute_masked_smooth_l1, compute_masked_smooth_l1_with_grad

    p, y, m = sl1_inputs(*shape, mask)
    l64, g64 = sl1_ref(p.double(), y.double(), m.double())
    l32, g32 = sl1_ref(p, y, m)
    loss, grad = compute_masked_smooth_l1_with_grad(p.to(DEV), y.to(DEV), m.to(DEV))
    if mask == "empty":
        assert float(loss) == 0.0 and not grad.any() and not torch.isnan(grad).any()
    else:
        check_against_f64(f"smooth_l1 {shape} {mask}", loss.cpu(), grad.cpu(), l64, g64, l32, g32)
    loss2, grad2 = compute_masked_smooth_l1_with_grad(p.to(DEV), y.to(DEV), m.to(DEV))
    assert torch.equal(loss, loss2) and torch.equal(grad, grad2)
    assert torch.equal(compute_masked_smooth_l1(p.to(DEV), y.to(DEV), m.to(DEV)), loss)


@pytest.mark.parametrize("name", LOSS_NAMES)
def test_loss_kernels_match_reference_record(name):
    """The recorded cases of the reference's own functions (float64 evaluation), same bars."""
    from sleap_nn_amd.training import losses as LS

    p = json.loads(str(Z[f"losses/{name}/params"]))
    t = {k: torch.from_numpy(Z[f"losses/{name}/{k}"]).to(DEV) for k in ("pred", "target", "mask") if f"losses/{name}/{k}" in Z.files}
    if p["kind"] == "bce_dice":
        loss, grad = LS.compute_bce_dice_loss_with_grad(t["pred"], t["target"], p["bce_weight"], p["dice_weight"], p["smooth"], p["pos_weight"])
    else:
        loss, grad = LS.compute_masked_smooth_l1_with_grad(t["pred"], t["target"], t["mask"])
    l64, g64 = torch.from_numpy(Z[f"losses/{name}/loss64"]), torch.from_numpy(Z[f"losses/{name}/grad64"])
    if float(l64) == 0.0:
        assert float(loss) == 0.0 and not grad.any()
    else:
        check_against_f64(name, loss.cpu(), grad.cpu(), l64, g64, torch.from_numpy(Z[f"losses/{name}/loss32"]), torch.from_numpy(Z[f"losses/{name}/grad32"]))


# ---- target kernels ------------------------------------------------------------------------------------------------------------------------

def render(masks, n, p):
    from sleap_nn_amd.data import segmentation_maps as SM

    hw = tuple(masks.shape[-2:])
    cent = SM.compute_mask_centroids(masks, n)
    fg = SM.generate_foreground_mask(masks, hw, output_stride=p["stride"], maxpool=p["maxpool"], n_instances=n)
    hm = SM.generate_center_heatmap(masks, hw, output_stride=p["stride"], sigma=p["sigma"], centers=cent, n_instances=n)
    off, wt = SM.generate_center_offsets(masks, hw, output_stride=p["stride"], centers=cent, n_instances=n)
    return fg, hm, off, wt, cent


@pytest.mark.parametrize("name", TARGET_NAMES)
def test_target_kernels_match_reference_and_cpu_form(name):
    p = json.loads(str(Z[f"targets/{name}/params"]))
    masks, n = torch.from_numpy(Z[f"targets/{name}/masks"]), torch.from_numpy(Z[f"targets/{name}/n_instances"])
    dev = [x.cpu() for x in render(masks.to(DEV), n.to(DEV), p)]
    cpu = render(masks, n, p)
    fg, hm, off, wt, cent = dev
    ref = {k: torch.from_numpy(Z[f"targets/{name}/{k}"]) for k in ("foreground", "center", "offsets", "weight", "centroids")}
    for other in (ref, dict(zip(("foreground", "center", "offsets", "weight", "centroids"), cpu))):
        assert torch.equal(fg, other["foreground"])
        assert torch.equal(wt, other["weight"])
        assert torch.equal(off, other["offsets"])  # one IEEE subtraction of identical operands
        assert torch.equal(torch.isnan(cent), torch.isnan(other["centroids"])) and torch.equal(torch.nan_to_num(cent), torch.nan_to_num(other["centroids"]))
        err = float((hm - other["center"]).abs().max())
        assert err <= 2e-6, (name, err)
    # centroids computed inside the heat-map / offset calls equal the ones handed in
    from sleap_nn_amd.data import segmentation_maps as SM

    md, nd = masks.to(DEV), n.to(DEV)
    assert torch.equal(SM.generate_center_heatmap(md, None, p["stride"], p["sigma"], n_instances=nd).cpu(), hm)
    off2, wt2 = SM.generate_center_offsets(md, None, p["stride"], n_instances=nd)
    assert torch.equal(off2.cpu(), off) and torch.equal(wt2.cpu(), wt)


def test_padding_slots_are_never_read():
    p = json.loads(str(Z["targets/padding_garbage/params"]))
    masks, n = torch.from_numpy(Z["targets/padding_garbage/masks"]), torch.from_numpy(Z["targets/padding_garbage/n_instances"])
    cleared = masks.clone()
    for b in range(masks.shape[0]):
        cleared[b, int(n[b]) :] = 0
    assert not torch.equal(cleared, masks)
    for a, b in zip(render(masks.to(DEV), n.to(DEV), p), render(cleared.to(DEV), n.to(DEV), p)):
        assert torch.equal(torch.nan_to_num(a), torch.nan_to_num(b))


# ---- training step -------------------------------------------------------------------------------------------------------------------------

def tiny_model(prefix):
    from sleap_nn_amd.architectures.model import Model

    cfg = json.loads(str(TINY[f"{prefix}/config_json"]))
    m = Model("unet", cfg["backbone"], cfg["heads"], cfg["model_type"])
    m.load_state_dict({k[len(prefix) + 3 :]: torch.from_numpy(TINY[k]) for k in TINY.files if k.startswith(f"{prefix}/w/")}, strict=True)
    return m, cfg


def step_batch(prefix):
    t = {k.split("/")[-1]: torch.from_numpy(Z[k]) for k in Z.files if k.startswith(f"step/{prefix}/target/")}
    batch = {"image": torch.from_numpy(Z[f"step/{prefix}/image"]), "SegmentationHead": t["foreground_mask"]}
    if prefix == "bu":
        batch.update({"InstanceCenterHead": t["center_heatmap"], "CenterOffsetHead": t["center_offsets"], "foreground_weight": t["foreground_weight"]})
    return batch


def check_grads(tm, ref_grads, rtol):
    got = tm.named_grads()
    assert set(got) == set(ref_grads)
    worst = 0.0
    for k, r in ref_grads.items():
        scale = max(float(r.abs().max()), 1e-12)
        err = float((got[k] - r).abs().max()) / scale
        worst = max(worst, err)
        assert err <= rtol, (k, err, scale)
    return worst


@pytest.mark.parametrize("prefix", ["bu", "sem"])
def test_training_step_matches_reference(prefix):
    from sleap_nn_amd.training.segmentation import SegmentationTrainingModule

    m, cfg = tiny_model(prefix)
    tm = SegmentationTrainingModule(m, DEV)
    assert (tm.bce_weight, tm.dice_weight, tm.bce_pos_weight) == (1.0, 1.0, None)  # the tiny configs carry non-default weights on purpose
    batch = step_batch(prefix)
    targets = {k: v for k, v in batch.items() if k != "image"}
    loss = tm.forward_backward(batch["image"], targets).cpu().numpy()
    ref = [float(Z[f"step/{prefix}/loss"])] + [float(Z[f"step/{prefix}/head_loss/{h.name}"]) for h in m.heads]
    print(prefix, "losses", loss.tolist(), "reference", ref)
    assert np.allclose(loss, np.array(ref, dtype=np.float32), rtol=2e-5, atol=0), (loss, ref)
    ref_grads = {k[len(f"step/{prefix}/grad/") :]: torch.from_numpy(Z[k]) for k in Z.files if k.startswith(f"step/{prefix}/grad/")}
    print(prefix, "worst gradient error relative to its tensor's scale", check_grads(tm, ref_grads, 2e-4))
    # in training the foreground head emits logits: their sigmoid, not they, is what the inference program returns (checked below)
    logits = tm._last_out["SegmentationHead"].clone()
    g1 = tm.grads.clone()
    tm.forward_backward(batch["image"], targets)
    assert torch.equal(g1, tm.grads)  # bitwise on a second run
    m.eval()
    probs = m(batch["image"].to(DEV))["SegmentationHead"]
    assert float(probs.min()) >= 0.0 and float(probs.max()) <= 1.0
    assert float((torch.sigmoid(logits) - probs).abs().max()) <= CMS_ATOL
    assert float((logits - probs).abs().max()) > 0.1  # (these weights give logits inside [0, 1]: told apart from probabilities by value, not by range)
    out = m(torch.from_numpy(TINY[f"{prefix}/image"]).squeeze(1).to(DEV))
    for k in [k for k in TINY.files if k.startswith(f"{prefix}/out/")]:
        err = float((out[k.split("/")[-1]].cpu() - torch.from_numpy(TINY[k])).abs().max())
        assert err <= CMS_ATOL, (k, err)
    tm.close()


@pytest.mark.parametrize("prefix", ["bu", "sem"])
def test_three_steps_on_generated_targets_lower_the_loss(prefix):
    from sleap_nn_amd.data.segmentation_maps import SegmentationTargetGenerator
    from sleap_nn_amd.training.segmentation import SegmentationTrainingModule

    m, cfg = tiny_model(prefix)
    tm = SegmentationTrainingModule(m, DEV, lr=1e-3)
    masks, n = torch.from_numpy(Z[f"step/{prefix}/masks"]).to(DEV), torch.from_numpy(Z[f"step/{prefix}/n_instances"]).to(DEV)
    targets = SegmentationTargetGenerator(cfg["model_type"], cfg["heads"])(masks, n)
    if prefix == "bu":
        assert targets["CenterOffsetHead"]._base is targets["foreground_weight"]._base  # rendered into one buffer: passed on without a copy
    batch = {"image": torch.from_numpy(Z[f"step/{prefix}/image"]), **targets}
    losses = [float(tm.training_step(batch)[0]) for _ in range(3)]
    losses.append(float(tm.validation_step(batch)[0]))
    print(prefix, "total loss over three steps, then validation", losses)
    assert losses[0] == pytest.approx(float(Z[f"step/{prefix}/loss"]), rel=2e-5)  # the generated targets are the recorded ones
    # each step reports the loss before its update: the three reported losses fall.  The loss after the third update is only held below the first one:
    # Adam's early updates move every parameter by about lr whatever the gradient's size, so a single step may overshoot
    assert losses[1] < losses[0] and losses[2] < losses[1] and losses[3] < losses[0]
    tm.close()


def test_plain_handles_are_still_refused():
    """Without a chosen head loss ``ph_model_backward`` refuses the program on the host, before anything is launched; ``TrainingModule`` refuses earlier."""
    from sleap_nn_amd import _lib as L
    from sleap_nn_amd.training.module import TrainingModule

    with pytest.raises(NotImplementedError, match="bottomup_segmentation"):
        TrainingModule(tiny_model("bu")[0], DEV)

    class OptsInButSetsNothing(TrainingModule):
        _trains_segmentation = True

    m, _ = tiny_model("sem")
    tm = OptsInButSetsNothing(m, DEV)
    batch = step_batch("sem")
    with pytest.raises(L.PosehipError, match="inference only"):
        tm.forward_backward(batch["image"], {"SegmentationHead": batch["SegmentationHead"]})
    tm.close()


def test_training_step_matches_independent_autograd():
    """A second shape, (48, 64) with B = 3 and random weights; the reference is ``oracle.cpu_ref.unet_forward`` plus the three 1x1 head convolutions
    written here plus the CPU forms of the losses, differentiated by torch autograd."""
    from sleap_nn_amd.architectures.model import Model
    from sleap_nn_amd.data.segmentation_maps import SegmentationTargetGenerator
    from sleap_nn_amd.training import losses as LS
    from sleap_nn_amd.training.segmentation import SegmentationTrainingModule

    bb = {"in_channels": 1, "kernel_size": 3, "filters": 8, "filters_rate": 2, "max_stride": 8, "stem_stride": None, "middle_block": True, "up_interpolate": True,
          "stacks": 1, "convs_per_block": 2, "output_stride": 2}
    heads = {"segmentation": {"output_stride": 2, "loss_weight": 1.0, "bce_weight": 0.7, "dice_weight": 0.3, "bce_pos_weight": 2.0},
             "center": {"sigma": 3.0, "output_stride": 2, "loss_weight": 0.8}, "offsets": {"output_stride": 2, "loss_weight": 0.1}}
    g = torch.Generator().manual_seed(23)
    pose = O.init_state(bb, {"confmaps": {"part_names": ["a"], "output_stride": 2}}, "single_instance", seed=23, head_scale=1.0)
    sd = {k: v for k, v in pose.items() if not k.startswith("head_layers.")}
    cin = next(v for k, v in pose.items() if k.startswith("head_layers.") and k.endswith(".weight")).shape[1]
    head_names = [("SegmentationHead", 1), ("InstanceCenterHead", 1), ("CenterOffsetHead", 2)]
    for i, (name, c) in enumerate(head_names):
        sd[f"head_layers.{i}.{name}.0.weight"] = (torch.rand((c, cin, 1, 1), generator=g) - 0.5) * (4.0 if i == 0 else 1.0)
    for k in list(sd):
        if k.endswith(".weight"):
            sd[k[: -len("weight")] + "bias"] = (torch.rand(sd[k].shape[0], generator=g) - 0.5) * 0.2
    B, H, W = 3, 48, 64
    img = torch.randint(0, 256, (B, 1, H, W), dtype=torch.uint8, generator=g)
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    masks = torch.zeros((B, 3, H, W), dtype=torch.uint8)
    for b, discs in enumerate((((20, 15, 9), (44, 30, 11)), (), ((30, 24, 13), (34, 22, 5), (10, 40, 4)))):  # (the second frame has no instance)
        for i, (cx, cy, r) in enumerate(discs):
            masks[b, i] = ((xx - cx) ** 2 + (yy - cy) ** 2 <= r * r).to(torch.uint8)
    n = torch.tensor([2, 0, 3], dtype=torch.int32)
    targets = SegmentationTargetGenerator("bottomup_segmentation", heads)(masks, n)  # the CPU form, pinned by the CPU tests

    params = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    feats = O.unet_forward(params, bb, O.normalize_input(img))
    x = feats["outputs"][feats["strides"].index(2)]
    out = {name: F.conv2d(x, params[f"head_layers.{i}.{name}.0.weight"], params[f"head_layers.{i}.{name}.0.bias"]) for i, (name, _) in enumerate(head_names)}
    hl = [LS.compute_bce_dice_loss(out["SegmentationHead"], targets["SegmentationHead"], 0.7, 0.3, 1.0, 2.0),
          F.mse_loss(out["InstanceCenterHead"], targets["InstanceCenterHead"]),
          LS.compute_masked_smooth_l1(out["CenterOffsetHead"], targets["CenterOffsetHead"], targets["foreground_weight"])]
    lw = [1.0, 0.8, 0.1]
    total = sum(w * l for w, l in zip(lw, hl))
    grads = torch.autograd.grad(total, list(params.values()))
    ref_grads = {k: gr.detach() for k, gr in zip(params, grads)}
    ref = [float(total.detach())] + [float(l.detach()) for l in hl]

    m = Model("unet", bb, heads, "bottomup_segmentation")
    m.load_state_dict(sd)
    tm = SegmentationTrainingModule(m, DEV)
    assert (tm.bce_weight, tm.dice_weight, tm.bce_pos_weight, tm.loss_weights) == (0.7, 0.3, 2.0, lw)
    loss = tm.forward_backward(img, dict(targets)).cpu().numpy()
    print("losses", loss.tolist(), "autograd", ref)
    assert np.allclose(loss, np.array(ref, dtype=np.float32), rtol=2e-5, atol=0), (loss, ref)
    print("worst gradient error relative to its tensor's scale", check_grads(tm, ref_grads, 2e-4))
    g1 = tm.grads.clone()
    tm.forward_backward(img, dict(targets))
    assert torch.equal(g1, tm.grads)
    tm.close()
