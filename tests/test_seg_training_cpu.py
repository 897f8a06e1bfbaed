"""Training of the segmentation model types without a GPU: the torch forms of the losses and of the mask targets against the reference's recorded
results (tests/golden/seg_training.npz, tools/gen_seg_training_golden.py), the target generator on the run directories, the ABI declarations, and
the refusals of ``SegmentationTrainingModule`` that need no device."""
import json
import os
import re

import numpy as np
import pytest
import torch

from tests import _golden as G

Z = G.load("seg_training.npz")
LOSS_NAMES = json.loads(str(Z["losses/names"]))
TARGET_NAMES = json.loads(str(Z["targets/names"]))
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CKPT_DIRS = os.path.join(ROOT, "tests", "golden", "ckpt_dirs")


def loss_case(name):
    p = json.loads(str(Z[f"losses/{name}/params"]))
    t = {k: torch.from_numpy(Z[f"losses/{name}/{k}"]) for k in ("pred", "target", "mask") if f"losses/{name}/{k}" in Z.files}
    return p, t


@pytest.mark.parametrize("name", LOSS_NAMES)
def test_cpu_losses_match_reference(name):
    from sleap_nn_amd.training import losses as LS

    p, t = loss_case(name)
    pred = t["pred"].clone().requires_grad_(True)
    if p["kind"] == "bce_dice":
        kw = dict(bce_weight=p["bce_weight"], dice_weight=p["dice_weight"], smooth=p["smooth"], pos_weight=p["pos_weight"])
        loss = LS.compute_bce_dice_loss(pred, t["target"], **kw)
        loss2, grad2 = LS.compute_bce_dice_loss_with_grad(t["pred"], t["target"], loss_weight=0.5, **kw)
    else:
        loss = LS.compute_masked_smooth_l1(pred, t["target"], t["mask"])
        loss2, grad2 = LS.compute_masked_smooth_l1_with_grad(t["pred"], t["target"], t["mask"], loss_weight=0.5)
    ref, ref_grad = float(Z[f"losses/{name}/loss32"]), torch.from_numpy(Z[f"losses/{name}/grad32"])
    assert float(loss.detach()) == pytest.approx(ref, rel=1e-6, abs=0.0 if ref == 0 else 1e-12)
    assert float(loss2) == pytest.approx(ref, rel=1e-6, abs=0.0 if ref == 0 else 1e-12)
    loss.backward()
    scale = max(float(ref_grad.abs().max()), 1e-12)
    assert float((pred.grad - ref_grad).abs().max()) <= 1e-6 * scale
    assert float((grad2 - 0.5 * ref_grad).abs().max()) <= 1e-6 * scale
    assert not torch.isnan(grad2).any()
    if name == "sl1_empty_mask":
        assert float(loss.detach()) == 0.0 and not pred.grad.any()


def test_loss_defaults_are_the_references():
    import inspect

    from sleap_nn_amd.training import losses as LS

    s = inspect.signature(LS.compute_bce_dice_loss)
    assert list(s.parameters) == ["y_pred", "y_gt", "bce_weight", "dice_weight", "smooth", "pos_weight"]
    assert [s.parameters[k].default for k in ("bce_weight", "dice_weight", "smooth", "pos_weight")] == [0.5, 0.5, 1.0, None]
    assert list(inspect.signature(LS.compute_masked_smooth_l1).parameters) == ["y_pred", "y_gt", "mask"]


def target_case(name):
    p = json.loads(str(Z[f"targets/{name}/params"]))
    return p, torch.from_numpy(Z[f"targets/{name}/masks"]), torch.from_numpy(Z[f"targets/{name}/n_instances"])


def check_targets(name, fg, hm, off, wt, cent):
    """Foreground, weight, offsets and centroids exactly equal the reference's; the heat map to 2e-6."""
    ref = {k: Z[f"targets/{name}/{k}"] for k in ("foreground", "center", "offsets", "weight", "centroids")}
    assert np.array_equal(fg.cpu().numpy(), ref["foreground"])
    assert np.array_equal(wt.cpu().numpy(), ref["weight"])
    assert np.array_equal(off.cpu().numpy(), ref["offsets"])
    assert np.array_equal(cent.cpu().numpy(), ref["centroids"], equal_nan=True)
    assert float(np.abs(hm.cpu().numpy() - ref["center"]).max()) <= 2e-6


def render(masks, n, p):
    from sleap_nn_amd.data import segmentation_maps as SM

    hw = tuple(masks.shape[-2:])
    cent = SM.compute_mask_centroids(masks, n)
    fg = SM.generate_foreground_mask(masks, hw, output_stride=p["stride"], maxpool=p["maxpool"], n_instances=n)
    hm = SM.generate_center_heatmap(masks, hw, output_stride=p["stride"], sigma=p["sigma"], centers=cent, n_instances=n)
    off, wt = SM.generate_center_offsets(masks, hw, output_stride=p["stride"], centers=cent, n_instances=n)
    return fg, hm, off, wt, cent


@pytest.mark.parametrize("name", TARGET_NAMES)
def test_cpu_targets_match_reference(name):
    p, masks, n = target_case(name)
    check_targets(name, *render(masks, n, p))


def test_padding_slots_are_ignored_and_empty_masks_are_not():
    p, masks, n = target_case("padding_garbage")
    a = render(masks, n, p)
    cleared = masks.clone()
    for b in range(masks.shape[0]):
        cleared[b, int(n[b]) :] = 0
    for x, y in zip(a, render(cleared, n, p)):
        assert torch.equal(torch.nan_to_num(x), torch.nan_to_num(y))
    # a real, empty mask: the image centre, and a Gaussian there
    p, masks, n = target_case("empty_real_mask")
    fg, hm, off, wt, cent = render(masks, n, p)
    H, W = masks.shape[-2:]
    assert cent[0, 1].tolist() == [W / 2.0, H / 2.0]
    assert float(hm[0, 0, H // 2 // p["stride"], W // 2 // p["stride"]]) > 0.9


def test_offsets_render_into_a_packed_buffer():
    from sleap_nn_amd.data import segmentation_maps as SM

    p, masks, n = target_case("blobs_s2")
    h, w = masks.shape[-2] // 2, masks.shape[-1] // 2
    buf = torch.full((1, 3, h, w), 7.0)
    off, wt = SM.generate_center_offsets(masks, None, output_stride=2, n_instances=n, out=buf)
    assert off.data_ptr() == buf.data_ptr() and wt._base is buf
    assert np.array_equal(buf[:, :2].numpy(), Z["targets/blobs_s2/offsets"]) and np.array_equal(buf[:, 2:].numpy(), Z["targets/blobs_s2/weight"])


@pytest.mark.parametrize("name,keys", [("tiny_bottomup_segmentation", {"SegmentationHead": 1, "InstanceCenterHead": 1, "CenterOffsetHead": 2, "foreground_weight": 1}),
                                       ("tiny_semantic_segmentation", {"SegmentationHead": 1})])
def test_target_generator_from_run_directory(name, keys):
    from sleap_nn_amd.data.segmentation_maps import SegmentationTargetGenerator
    from sleap_nn_amd.data.targets import TargetGenerator

    tg = SegmentationTargetGenerator.from_training_config(os.path.join(CKPT_DIRS, name))
    masks, n = torch.from_numpy(Z["step/bu/masks"]), torch.from_numpy(Z["step/bu/n_instances"])
    out = tg(masks, n)
    B, _, H, W = masks.shape
    assert set(out) == set(keys)
    for k, c in keys.items():
        assert tuple(out[k].shape) == (B, c, H // 2, W // 2) and out[k].dtype == torch.float32, k
    with pytest.raises(NotImplementedError):  # the pose generator keeps refusing these types
        TargetGenerator.from_training_config(os.path.join(CKPT_DIRS, name))
    with pytest.raises(NotImplementedError):
        SegmentationTargetGenerator("centered_instance_segmentation", {"segmentation": {"output_stride": 2}})
    with pytest.raises(NotImplementedError):
        SegmentationTargetGenerator("bottomup", {})


def test_target_generator_reproduces_the_step_targets():
    """The recorded batches of the reference's training steps are what the generator renders from the same masks (heat map to 2e-6)."""
    from sleap_nn_amd.data.segmentation_maps import SegmentationTargetGenerator

    cfg = json.loads(str(G.load("unet_tiny_seg.npz")["bu/config_json"]))
    out = SegmentationTargetGenerator("bottomup_segmentation", cfg["heads"])(torch.from_numpy(Z["step/bu/masks"]), torch.from_numpy(Z["step/bu/n_instances"]))
    for ours, theirs in (("SegmentationHead", "foreground_mask"), ("CenterOffsetHead", "center_offsets"), ("foreground_weight", "foreground_weight")):
        assert np.array_equal(out[ours].numpy(), Z[f"step/bu/target/{theirs}"]), ours
    assert float(np.abs(out["InstanceCenterHead"].numpy() - Z["step/bu/target/center_heatmap"]).max()) <= 2e-6
    assert out["CenterOffsetHead"]._base is out["foreground_weight"]._base  # one (B, 3, h, w) buffer


def test_target_maxpool_is_read_from_the_head_config():
    from sleap_nn_amd.data.segmentation_maps import SegmentationTargetGenerator

    p, masks, n = target_case("line_s4_maxpool")
    for flag, case in ((True, "line_s4_maxpool"), (False, "line_s4")):
        tg = SegmentationTargetGenerator("semantic_segmentation", {"segmentation": {"output_stride": 4, "target_maxpool": flag}})
        assert np.array_equal(tg(masks, n)["SegmentationHead"].numpy(), Z[f"targets/{case}/foreground"])


def test_abi_declarations_are_consistent():
    from sleap_nn_amd import _lib as L
    from sleap_nn_amd import build as B

    with open(os.path.join(ROOT, "include", "posehip.h")) as f:
        header = f.read()
    new = ("ph_model_set_head_loss", "ph_loss_scratch_bytes", "ph_loss_bce_dice", "ph_loss_masked_smooth_l1", "ph_render_seg_targets")
    for name in new:
        m = re.search(r"^(?:int|int64_t)\s+" + name + r"\s*\(([^;]*)\)\s*;", header, re.M)
        assert m, f"{name} is not declared in include/posehip.h"
        assert name in L.SIGNATURES, name
        n_args = len([a for a in m.group(1).split(",") if a.strip() and a.strip() != "void"])
        assert n_args == len(L.SIGNATURES[name][1]), (name, n_args, len(L.SIGNATURES[name][1]))
    for k, v in (("PH_LOSS_MSE", L.LOSS_MSE), ("PH_LOSS_BCE_DICE", L.LOSS_BCE_DICE), ("PH_LOSS_MASKED_SMOOTH_L1", L.LOSS_MASKED_SMOOTH_L1)):
        assert int(re.search(r"^#define\s+" + k + r"\s+(\d+)", header, re.M).group(1)) == v
    assert int(re.search(r"^#define\s+PH_VERSION\s+(\d+)", header, re.M).group(1)) >= 113
    assert "seg_loss_kernels.hip" in B.SOURCES and "seg_target_kernels.hip" in B.SOURCES
    lib = L.lib()  # the built library exports them and reports the header's version
    for name in new:
        assert hasattr(lib, name)
    assert lib.ph_version() == int(re.search(r"^#define\s+PH_VERSION\s+(\d+)", header, re.M).group(1))
    assert lib.ph_loss_scratch_bytes(2, 2) > 0 and lib.ph_loss_scratch_bytes(0, 1) < 0


def _model(prefix="bu"):
    from sleap_nn_amd.architectures.model import Model

    cfg = json.loads(str(G.load("unet_tiny_seg.npz")[f"{prefix}/config_json"]))
    return Model("unet", cfg["backbone"], cfg["heads"], cfg["model_type"])


def test_module_refusals_need_no_device():
    from sleap_nn_amd import _lib as L
    from sleap_nn_amd.architectures.model import Model
    from sleap_nn_amd.training.module import OHKMConfig, TrainingModule
    from sleap_nn_amd.training.segmentation import SegmentationTrainingModule

    assert issubclass(SegmentationTrainingModule, TrainingModule)
    with pytest.raises(ValueError, match="hard keypoint"):
        SegmentationTrainingModule(_model(), ohkm=OHKMConfig(online_mining=True))
    with pytest.raises(ValueError, match="negative_loss_weight"):
        SegmentationTrainingModule(_model(), negative_loss_weight=0.5)
    bb = {"in_channels": 1, "kernel_size": 3, "filters": 8, "filters_rate": 2, "max_stride": 8, "stem_stride": None, "middle_block": True, "up_interpolate": True,
          "stacks": 1, "convs_per_block": 2, "output_stride": 2}
    pose = Model("unet", bb, {"confmaps": {"part_names": ["a", "b"], "output_stride": 2}}, "single_instance")
    with pytest.raises(ValueError, match="single_instance"):
        SegmentationTrainingModule(pose)
    with pytest.raises(NotImplementedError, match="bottomup_segmentation"):  # the base class keeps refusing
        TrainingModule(_model())
    # a fresh model still carries the refusal flag on every head op, and remembers nothing until a module chooses the losses
    m = _model()
    assert all(o.flags & L.FLAG_NO_TRAIN for o in m.ops if o.kind == L.OP_HEAD) and m._head_losses == {}
    m.set_head_loss(0, L.LOSS_BCE_DICE, (1.0, 1.0, 1.0, -1.0))
    assert m._head_losses == {0: (L.LOSS_BCE_DICE, (1.0, 1.0, 1.0, -1.0))}
