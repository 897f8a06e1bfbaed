"""Targets of the identity and top-down model types on the GPU: ph_render_class_maps / ph_instance_centroids / ph_render_confmaps through
sleap_nn_amd/data/targets.py against the reference's recorded results (tests/golden/targets_identity.npz), against the module's CPU
implementation on a larger random case, and end to end through a training step.

Bounds.  Confidence maps: 2e-6 absolute, the project's rendering bar (expf vs torch.exp).  Class maps: ``2e-6 * (1 + I) / threshold`` -- a map
value M_i and the sum S of I of them carry the rendering error e and I * e, and mask = M_i / S is taken only where S >= M_i > threshold, so
|d mask| <= (e + (M_i / S) * I * e) / S <= e * (1 + I) / threshold.  Centroids: anchors bit for bit, the mean fallback 1e-6 absolute (a float sum
of at most N terms divided once, summed in the host's order).

Each test prints its largest error per case before it asserts; the measured figures are in DESIGN.md section 11."""
import json

import numpy as np
import pytest
import torch

from oracle import cpu_ref as O
from tests import _golden as G

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def gold():
    return G.load("targets_identity.npz")


def _names(z, group):
    return json.loads(str(z[f"{group}/names"]))


def class_map_bound(I, threshold):
    return 2e-6 * (1 + I) / threshold


def test_class_maps_kernel_matches_the_goldens(gold):
    from sleap_nn_amd.data.targets import generate_class_maps

    for name in _names(gold, "class_maps"):
        p = json.loads(str(gold[f"class_maps/{name}/params"]))
        pts, cls, exp = (gold[f"class_maps/{name}/{k}"] for k in ("points", "class_inds", "expected"))
        kw = dict(class_map_threshold=p["class_map_threshold"], sigma=p["sigma"], output_stride=p["output_stride"], is_centroids=p["is_centroids"])
        dev = generate_class_maps(torch.from_numpy(pts).to(DEV), p["img_hw"], torch.from_numpy(cls).to(DEV), p["num_tracks"], **kw)
        out = dev.cpu().numpy()
        assert out.shape == exp.shape and not np.isnan(out).any(), name
        err, bound = float(np.abs(out - exp).max()), class_map_bound(cls.shape[1], p["class_map_threshold"])
        print(f"class maps [{name}]: max error {err:.2e} (bound {bound:.1e})")
        assert err <= bound, (name, err, bound)
        again = generate_class_maps(torch.from_numpy(pts).to(DEV), p["img_hw"], torch.from_numpy(cls).to(DEV), p["num_tracks"], **kw)
        assert torch.equal(dev, again), name  # a second launch: bit for bit


def test_class_maps_kernel_edge_contracts():
    from sleap_nn_amd import _lib as L
    from sleap_nn_amd.data.targets import generate_class_maps

    hw = (12, 20)
    nan = float("nan")
    out = generate_class_maps(torch.full((1, 2, 1, 2), nan, device=DEV), hw, torch.tensor([[0, 1]], device=DEV), 2)  # S = 0 everywhere
    assert out.shape == (1, 2, 6, 10) and float(out.abs().max()) == 0.0
    pts = torch.tensor([[[[4.0, 4.0]], [[nan, nan]]]], device=DEV)
    out = generate_class_maps(pts, hw, torch.tensor([[1, 0]], device=DEV), 2)
    assert float(out[0, 1, 2, 2]) == 1.0 and float(out[0, 0].max()) == 0.0
    assert float(generate_class_maps(pts, hw, torch.tensor([[-1, -1]], device=DEV), 3).abs().max()) == 0.0
    out = generate_class_maps(torch.zeros((2, 0, 3, 2), device=DEV), hw, torch.zeros((2, 0), dtype=torch.int32, device=DEV), 2)  # no instance rows at all
    assert out.shape == (2, 2, 6, 10) and float(out.abs().max()) == 0.0
    out = generate_class_maps(torch.zeros((0, 2, 3, 2), device=DEV), hw, torch.zeros((0, 2), dtype=torch.int32, device=DEV), 2)  # an empty batch: as on the CPU
    assert out.shape == (0, 2, 6, 10) and out.is_cuda
    from sleap_nn_amd.data.targets import generate_confmaps

    assert generate_confmaps(torch.zeros((0, 3, 2), device=DEV), hw).shape == (0, 3, 6, 10)
    with pytest.raises(L.PosehipError):  # a frame that does not fit the staged LDS is refused, not truncated
        generate_class_maps(torch.zeros((1, 700, 12, 2), device=DEV), hw, torch.zeros((1, 700), dtype=torch.int32, device=DEV), 2)


def test_centroid_and_confmap_kernels_match_the_goldens(gold):
    from sleap_nn_amd.data.targets import generate_centroids, generate_confmaps

    for name in _names(gold, "centroids"):
        anchor = json.loads(str(gold[f"centroids/{name}/params"]))["anchor_ind"]
        pts, exp = gold[f"centroids/{name}/points"], gold[f"centroids/{name}/expected"]
        dev = generate_centroids(torch.from_numpy(pts).to(DEV), anchor_ind=anchor)
        out = dev.cpu().numpy()
        assert out.shape == exp.shape and np.array_equal(np.isnan(out), np.isnan(exp)), name
        if anchor is not None:
            rows = ~np.isnan(pts[:, anchor]).any(-1)
            assert np.array_equal(out[rows], pts[rows, anchor]), name  # anchors: bit for bit
        err = float(np.nanmax(np.abs(out - exp), initial=0.0))
        print(f"centroids [{name}]: max error {err:.2e}")
        assert err <= 1e-6, (name, err)
        assert torch.equal(dev.nan_to_num(-1.0), generate_centroids(torch.from_numpy(pts).to(DEV), anchor_ind=anchor).nan_to_num(-1.0))
    for name in _names(gold, "confmaps"):
        p = json.loads(str(gold[f"confmaps/{name}/params"]))
        pts, exp = gold[f"confmaps/{name}/points"], gold[f"confmaps/{name}/expected"]
        out = generate_confmaps(torch.from_numpy(pts).to(DEV), p["img_hw"], sigma=p["sigma"], output_stride=p["output_stride"]).cpu().numpy()
        assert out.shape == exp.shape
        print(f"confmaps [{name}]: max error {float(np.abs(out - exp).max()):.2e}")
        np.testing.assert_allclose(out, exp, rtol=0, atol=2e-6)


def test_device_and_cpu_implementations_agree_on_a_random_case():
    """B = 4, I = 9, N = 13, C = 6 at 250 x 282, stride 4: more than one workgroup per frame, a grid that is no multiple of a wave, I > C.  The seed is one
    whose per-instance maps all stay 1e-4 clear of the threshold (asserted: the class map is discontinuous there)."""
    from sleap_nn_amd.data.targets import _gaussians, generate_centroids, generate_class_maps, generate_confmaps

    B, I, N, Cn, hw, stride, sigma, thr = 4, 9, 13, 6, (250, 282), 4, 2.0, 0.2
    gen = torch.Generator().manual_seed(57)
    centre = torch.rand((B, I, 1, 2), generator=gen) * torch.tensor([300.0, 260.0]) - 10.0
    pts = centre + torch.randn((B, I, N, 2), generator=gen) * 12.0
    pts[torch.rand((B, I, N), generator=gen) < 0.15] = float("nan")
    pts[1, 4] = float("nan")
    pts[2, 0, 3, 1] = float("nan")
    cls = torch.randint(-1, Cn, (B, I), generator=gen)
    m64 = _gaussians(pts.double(), hw, sigma, stride).amax(dim=2)
    assert float((m64 - thr).abs().min()) >= 1e-4
    cpu = generate_class_maps(pts, hw, cls, Cn, class_map_threshold=thr, sigma=sigma, output_stride=stride)
    dev = generate_class_maps(pts.to(DEV), hw, cls.to(DEV), Cn, class_map_threshold=thr, sigma=sigma, output_stride=stride)
    assert cpu.shape == (B, Cn, 63, 71) and float((cpu > 0).float().mean()) > 0.01
    err = float((dev.cpu() - cpu).abs().max())
    print(f"class maps, device vs CPU: max error {err:.2e} (bound {class_map_bound(I, thr):.1e})")
    assert err <= class_map_bound(I, thr)
    assert torch.equal(dev, generate_class_maps(pts.to(DEV), hw, cls.to(DEV), Cn, class_map_threshold=thr, sigma=sigma, output_stride=stride))
    for anchor in (None, 3):
        c_cpu, c_dev = generate_centroids(pts, anchor), generate_centroids(pts.to(DEV), anchor).cpu()
        assert torch.equal(torch.isnan(c_cpu), torch.isnan(c_dev)) and bool(torch.isnan(c_cpu[1, 4]).all())
        err = float((c_cpu - c_dev).nan_to_num(0.0).abs().max())
        print(f"centroids (anchor {anchor}), device vs CPU: max error {err:.2e}")
        assert err <= 1e-6  # (below one ulp of these coordinates: holds because instance_centroids_kernel sums in the order of THIS torch's CPU sum over a strided
        # axis -- four interleaved partial sums, ATen's 16-term cascade; a torch whose reduction order differs shows here first)
    for p in (pts[:, 0], pts):
        c_cpu, c_dev = generate_confmaps(p, hw, sigma, stride), generate_confmaps(p.to(DEV), hw, sigma, stride).cpu()
        assert c_cpu.shape == c_dev.shape == (B, p.numel() // (2 * B), 63, 71)
        torch.testing.assert_close(c_dev, c_cpu, rtol=0, atol=2e-6)


def test_class_maps_kernel_with_long_staging_loops_and_a_grid_stride():
    """The paths the small cases do not reach: a frame's points (I * N * 2 = 264 floats) and weights (C * I = 264) each take more than one pass of the 256 staging
    threads, and with B = 96 frames a workgroup owns more than one chunk of 256 grid points (a frame gets about 8 workgroups per CU / B = 22 of them on 256 CUs, the
    80 x 80 map has 25 chunks), against the CPU implementation at the class-map bound.  Coordinates are integers at stride 1 with sigma 2, so every map value is
    exp(-k / 8) for an integer k: the nearest to the threshold 0.2 are k = 12 (0.223) and k = 13 (0.197), and no seed has to be chosen."""
    from sleap_nn_amd.data.targets import generate_class_maps

    B, I, N, Cn, hw, thr = 96, 33, 4, 8, (80, 80), 0.2
    gen = torch.Generator().manual_seed(3)
    pts = torch.randint(-3, 84, (B, I, N, 2), generator=gen).float()
    pts[torch.rand((B, I, N), generator=gen) < 0.2] = float("nan")
    pts[5] = float("nan")
    cls = torch.randint(-1, Cn, (B, I), generator=gen)
    kw = dict(class_map_threshold=thr, sigma=2.0, output_stride=1)
    cpu = torch.cat([generate_class_maps(pts[b : b + 16], hw, cls[b : b + 16], Cn, **kw) for b in range(0, B, 16)])
    dev = generate_class_maps(pts.to(DEV), hw, cls.to(DEV), Cn, **kw)
    assert dev.shape == cpu.shape == (B, Cn, 80, 80) and float((cpu > 0).float().mean()) > 0.01 and float(cpu[5].abs().max()) == 0.0
    err = float((dev.cpu() - cpu).abs().max())
    print(f"class maps, B = 96, I = 33: max error {err:.2e} (bound {class_map_bound(I, thr):.1e})")
    assert err <= class_map_bound(I, thr)
    assert torch.equal(dev, generate_class_maps(pts.to(DEV), hw, cls.to(DEV), Cn, **kw))


def test_multi_class_bottomup_training_step_on_device_rendered_targets():
    """Points on the device -> TargetGenerator -> TrainingModule.forward_backward, against the oracle's autograd step fed the CPU-rendered targets
    (tolerances of tests/test_gpu_training.py: loss 1e-5 relative, gradients 1e-4 of each tensor's scale)."""
    from sleap_nn_amd.architectures.model import Model
    from sleap_nn_amd.data import TargetGenerator
    from sleap_nn_amd.training.module import TrainingModule

    bb = {"in_channels": 1, "kernel_size": 3, "filters": 8, "filters_rate": 2, "max_stride": 8, "stem_stride": None, "middle_block": True,
          "up_interpolate": True, "stacks": 1, "convs_per_block": 2, "output_stride": 2}
    names = ["n0", "n1", "n2"]
    heads = {"confmaps": {"part_names": names, "sigma": 1.5, "output_stride": 2, "loss_weight": 1.0},
             "class_maps": {"classes": ["a", "b"], "sigma": 2.0, "output_stride": 4, "loss_weight": 0.6}}
    mt, hw, B = "multi_class_bottomup", (48, 64), 2
    sd = O.init_state(bb, heads, mt, seed=13, head_scale=1.0)
    g = torch.Generator().manual_seed(13)
    img = torch.randint(0, 256, (B, 1, hw[0], hw[1]), dtype=torch.uint8, generator=g)
    pts = torch.rand((B, 3, 3, 2), generator=g) * torch.tensor([64.0, 48.0])
    pts[1, 2] = float("nan")
    pts[0, 1, 2] = float("nan")
    cls = torch.tensor([[1, 0, 1], [0, 1, -1]])
    tg = TargetGenerator(mt, heads)
    t_cpu = tg(pts, hw, cls)
    t_dev = tg(pts.to(DEV), hw, cls.to(DEV))
    assert set(t_dev) == {"MultiInstanceConfmapsHead", "ClassMapsHead"} and all(v.is_cuda for v in t_dev.values())
    assert tuple(t_dev["ClassMapsHead"].shape) == (B, 2, 12, 16) and float(t_cpu["ClassMapsHead"].max()) > 0.5
    m = Model("unet", bb, heads, mt)
    m.load_state_dict(sd)
    lw = [h.loss_weight for h in m.heads]
    tm = TrainingModule(m, DEV, loss_weights=lw)
    ref_losses, ref_grads = O.training_step(sd, bb, heads, mt, img, t_cpu, lw)
    loss = tm.forward_backward(img, t_dev).cpu().numpy()
    assert np.allclose(loss, np.array(ref_losses, dtype=np.float32), rtol=1e-5, atol=1e-7), (loss, ref_losses)
    got = tm.named_grads()
    assert set(got) == set(ref_grads)
    for k, r in ref_grads.items():
        scale = max(float(r.abs().max()), 1e-12)
        assert float((got[k] - r).abs().max()) / scale <= 1e-4, k
