"""GPU parity of the training step (forward + MSE/OHKM + backward + Adam) against the oracle's
torch-autograd restatement of the reference step.  Tolerances: loss 1e-5 relative; gradients
1e-4 relative to each tensor's max magnitude (fp32, different summation orders)."""
import numpy as np
import pytest
import torch

from oracle import cpu_ref as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _cfg(filters=8, max_stride=8, output_stride=2, in_ch=1, bottomup=True, n_nodes=3):
    bb = {"in_channels": in_ch, "kernel_size": 3, "filters": filters, "filters_rate": 2, "max_stride": max_stride, "stem_stride": None, "middle_block": True,
          "up_interpolate": True, "stacks": 1, "convs_per_block": 2, "output_stride": output_stride}
    names = [f"n{i}" for i in range(n_nodes)]
    if bottomup:
        heads = {"confmaps": {"part_names": names, "output_stride": output_stride, "loss_weight": 1.0},
                 "pafs": {"edges": [[names[i], names[i + 1]] for i in range(n_nodes - 1)], "output_stride": output_stride * 2, "loss_weight": 0.7}}
        return bb, heads, "bottomup"
    return bb, {"confmaps": {"part_names": names, "output_stride": output_stride, "loss_weight": 1.0}}, "single_instance"


def _setup(bb, heads, mt, hw, B, seed, **kw):
    from sleap_nn_amd.architectures.model import Model
    from sleap_nn_amd.training.module import TrainingModule

    sd = O.init_state(bb, heads, mt, seed=seed, head_scale=1.0)
    g = torch.Generator().manual_seed(seed)
    for k in sd:
        if k.endswith(".bias"):
            sd[k] = (torch.rand(sd[k].shape, generator=g) - 0.5) * 0.2
    img = torch.randint(0, 256, (B, bb["in_channels"], hw[0], hw[1]), dtype=torch.uint8, generator=g)
    ref_out = O.model_forward(sd, bb, heads, mt, img)
    targets = {k: torch.rand(v.shape, generator=g) * 0.5 for k, v in ref_out.items()}
    m = Model("unet", bb, heads, mt)
    m.load_state_dict(sd)
    lw = [h.loss_weight for h in m.heads]
    tm = TrainingModule(m, DEV, loss_weights=lw, **kw)
    return sd, img, targets, lw, tm


def _check_grads(tm, ref_grads, rtol=1e-4):
    got = tm.named_grads()
    assert set(got) == set(ref_grads)
    worst = 0.0
    for k, r in ref_grads.items():
        scale = max(float(r.abs().max()), 1e-12)
        err = float((got[k] - r).abs().max()) / scale
        worst = max(worst, err)
        assert err <= rtol, (k, err, scale)
    return worst


@pytest.mark.parametrize("case", ["bottomup_small", "single_rgb", "wide_channels", "odd_batch"])
def test_backward_matches_autograd(case):
    if case == "bottomup_small":
        bb, heads, mt = _cfg(8, 8, 2)
        hw, B = (48, 64), 2
    elif case == "single_rgb":
        bb, heads, mt = _cfg(8, 4, 1, in_ch=3, bottomup=False)
        hw, B = (32, 40), 2
    elif case == "wide_channels":  # exercises the BN=64 / LDS-DMA dgrad path and 32-wide wgrad tiles with padding
        bb, heads, mt = _cfg(24, 16, 4)
        hw, B = (64, 96), 2
    else:
        bb, heads, mt = _cfg(16, 32, 4)
        hw, B = (64, 64), 3
    sd, img, targets, lw, tm = _setup(bb, heads, mt, hw, B, seed=11)
    ref_losses, ref_grads = O.training_step(sd, bb, heads, mt, img, targets, lw)
    loss = tm.forward_backward(img, targets).cpu().numpy()
    assert np.allclose(loss, np.array(ref_losses, dtype=np.float32), rtol=1e-5, atol=1e-7), (loss, ref_losses)
    _check_grads(tm, ref_grads)
    # determinism: bitwise identical gradients on a second run
    g1 = tm.grads.clone()
    tm.forward_backward(img, targets)
    assert torch.equal(g1, tm.grads)


def test_ohkm_loss_and_grads():
    bb, heads, mt = _cfg(8, 8, 2, n_nodes=5)
    from sleap_nn_amd.training.module import OHKMConfig

    sd, img, targets, lw, tm = _setup(bb, heads, mt, (48, 64), 2, seed=5, ohkm=OHKMConfig(online_mining=True, hard_to_easy_ratio=1.05, min_hard_keypoints=2, loss_scale=5.0))
    ref_losses, ref_grads = O.training_step(sd, bb, heads, mt, img, targets, lw, ohkm={"hard_to_easy_ratio": 1.05, "min_hard_keypoints": 2, "max_hard_keypoints": None, "loss_scale": 5.0})
    loss = tm.forward_backward(img, targets).cpu().numpy()
    assert np.allclose(loss, np.array(ref_losses, dtype=np.float32), rtol=1e-5), (loss, ref_losses)
    _check_grads(tm, ref_grads)


def test_adam_steps_match_torch_optim():
    """Three optimizer steps against the oracle's torch.optim restatement, two ways.
    (a) End to end -- oracle gradients -> oracle Adam vs device gradients -> device Adam -- at 2e-6, with the direct nine-tap
        weight-gradient kernel (wgrad_wino = 0).  Adam's first steps are lr * g / (|g| + 1e-8): an element whose gradient is
        within ~1e-7 of zero moves by a visible fraction of lr when the gradient changes by 1e-8, so this comparison measures the
        conv kernels' ABSOLUTE rounding noise, not the optimizer.  The Winograd-domain weight gradient (default; 4/9 of the
        matrix work) is as close to the float64 gradient as the direct kernel on every tensor (tools/wgrad_accuracy.py: same
        errors to three digits) but its noise floor on near-zero elements is ~1e-8 of the tensor scale instead of ~1e-10
        (sums of transformed, i.e. 4 - 16x larger, products that cancel in G^T . G).
    (b) Default kernels: the Adam arithmetic itself on the DEVICE's own gradients (exactly what the optimizer kernel consumed) at
        the same 2e-6, and the end-to-end parameters within 1e-4 = a tenth of one lr step (measured worst 4.5e-5)."""
    bb, heads, mt = _cfg(8, 8, 2)
    for amsgrad, optimizer in ((False, "Adam"), (True, "Adam"), (False, "AdamW")):
        for wgrad_wino in (0, 1):
            sd, img, targets, lw, tm = _setup(bb, heads, mt, (48, 64), 2, seed=3, lr=1e-3, amsgrad=amsgrad, optimizer=optimizer)
            tm.model.set_option("wgrad_wino", wgrad_wino)
            grads_seq, dev_seq, cur = [], [], {k: v.clone() for k, v in sd.items()}
            for step in range(3):
                _, g = O.training_step(cur, bb, heads, mt, img, targets, lw)
                grads_seq.append(g)
                cur = O.adam_reference(sd, grads_seq, lr=1e-3, amsgrad=amsgrad, optimizer=optimizer)
                tm.training_step({"image": img, **targets})
                dev_seq.append({k: v.clone() for k, v in tm.named_grads().items()})
            got = tm.state_dict()
            own = O.adam_reference(sd, dev_seq, lr=1e-3, amsgrad=amsgrad, optimizer=optimizer)
            for k, r in cur.items():
                assert torch.allclose(got[k], own[k], atol=2e-6, rtol=1e-4), (k, float((got[k] - own[k]).abs().max()))
                if wgrad_wino == 0:
                    assert torch.allclose(got[k], r, atol=2e-6, rtol=1e-4), (k, float((got[k] - r).abs().max()))
                else:
                    assert torch.allclose(got[k], r, atol=1e-4, rtol=1e-4), (k, float((got[k] - r).abs().max()))
            # the re-packed device weights are what the next forward uses
            out = tm.model.forward(img.to(DEV))
            ref = O.model_forward(cur, bb, heads, mt, img)
            for k, v in ref.items():
                assert (out[k].cpu() - v).abs().max().item() <= 1e-4


def test_training_reduces_loss():
    bb, heads, mt = _cfg(8, 8, 2, bottomup=False)
    sd, img, targets, lw, tm = _setup(bb, heads, mt, (32, 32), 4, seed=9, lr=3e-3)
    losses = [float(tm.training_step({"image": img, **targets})[0]) for _ in range(30)]
    assert losses[-1] < 0.5 * losses[0], losses[::5]


def test_data_parallel_gradient_equivalence():
    """DDP semantics without a second GPU: the mean of the gradients of two equal shards (what the
    flat all-reduce + 1/world_size produces) equals the gradient of the full batch, because every
    head loss is a mean over all elements."""
    bb, heads, mt = _cfg(8, 8, 2)
    sd, img, targets, lw, tm = _setup(bb, heads, mt, (48, 64), 4, seed=21)
    tm.forward_backward(img, targets)
    full = tm.grads.clone()
    acc = torch.zeros_like(full)
    for r in range(2):
        sl = slice(2 * r, 2 * r + 2)
        tm.forward_backward(img[sl], {k: v[sl] for k, v in targets.items()})
        acc += tm.grads
    acc /= 2
    scale = float(full.abs().max())
    assert float((acc - full).abs().max()) <= 1e-5 * scale


def test_native_rccl_exchange_runs_the_two_bucket_schedule_inside_the_backward():
    """SURVEY 8(b) `ph_allreduce` / VERDICT r5 item 6: the gradient exchange behind the C ABI.  One GPU admits one RCCL rank, so this is the single-rank communicator:
    ncclGetUniqueId -> ncclCommInitRank(world 1) through ph_comm_*; ph_allreduce sums a buffer over one rank (unchanged); and ph_model_backward with the communicator
    attached (ph_model_set_comm) runs its whole schedule -- tail bucket on the side stream behind the mid-sweep event, head bucket behind the sweep, the caller's stream
    joined -- and leaves the SAME gradients bit for bit, then trains as before.  (The multi-rank arithmetic -- sum x 1 / world == the global-batch gradient -- is the
    gloo world-size-2 test of tests/test_parallel_cpu.py; the multi-GPU run is the driver's.)"""
    import ctypes as C

    from sleap_nn_amd import _lib as L
    from sleap_nn_amd.parallel import Communicator

    assert Communicator.available(), "librccl could not be opened on the GPU box"
    comm = Communicator.create(torch.device(DEV))
    assert comm.world == 1 and L.lib().ph_comm_world(C.c_void_p(comm.handle)) == 1
    buf = torch.randn(1 << 20, device=DEV)
    ref = buf.clone()
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream())
    comm.all_reduce_(buf, stream=side)
    side.synchronize()
    assert torch.equal(buf, ref)
    bb, heads, mt = _cfg(8, 8, 2)
    sd, img, targets, lw, tm = _setup(bb, heads, mt, (48, 64), 4, seed=21)
    tm.forward_backward(img, targets)
    torch.cuda.synchronize()
    plain = tm.grads.clone()
    split = int(L.lib().ph_model_grad_bucket_split(tm.model._handle))
    assert 0 < split < tm.grads.numel()  # the arena of this network splits: both buckets are exercised
    tm._comm, tm._comm_stream = comm, side
    tm.forward_backward(img, targets)
    torch.cuda.synchronize()
    assert torch.equal(tm.grads, plain)
    assert tm.all_reduce_grads() == 1.0
    losses = [float(tm.training_step({"image": img, **targets})[0]) for _ in range(12)]
    assert losses[-1] < losses[0]
    tm.close()  # unbinds and destroys the communicator
    assert tm._comm is None
    tm.forward_backward(img, targets)  # ... and the handle runs without one again


def test_target_rendering_matches_reference_and_oracle():
    """ph_render_confmaps / ph_render_pafs vs the reference fixture (tests/golden/targets.npz) and, on a
    larger random case with many instances, vs the oracle.  fp32 tolerance 2e-6 abs (expf vs torch.exp)."""
    import json

    from sleap_nn_amd.data.targets import generate_multiconfmaps, generate_pafs
    from tests import _golden as G

    g = G.load("targets.npz")
    meta = json.loads(str(g["meta_json"]))
    pts = torch.from_numpy(g["points"]).cuda()
    for stride, sigma in meta["confmaps"]:
        out = generate_multiconfmaps(pts, meta["hw"], sigma=sigma, output_stride=stride).cpu().numpy()
        np.testing.assert_allclose(out, g[f"confmaps_s{stride}"], rtol=0, atol=2e-6)
    for stride, sigma in meta["pafs"]:
        out = generate_pafs(pts, meta["hw"], sigma=sigma, output_stride=stride, edge_inds=meta["edges"]).cpu().numpy()
        np.testing.assert_allclose(out, g[f"pafs_s{stride}"], rtol=0, atol=5e-6)

    # the reference's own known-answer vectors (tests/data/test_edge_maps.py:65-167)
    from tests.test_oracle_golden import _PAF_KAT

    inst = torch.tensor([[[[1.0, 0.5], [1.0, 1.5], [0.0, 0.0], [2.0, 2.0]]]]).cuda()
    np.testing.assert_allclose(generate_pafs(inst, (3, 3), sigma=1.0, output_stride=1, edge_inds=[(0, 1), (2, 3)]).cpu().numpy().reshape(2, 2, 3, 3), _PAF_KAT, atol=1e-3)
    np.testing.assert_allclose(generate_pafs(inst.repeat(1, 2, 1, 1), (3, 3), sigma=1.0, output_stride=1, edge_inds=[(0, 1), (2, 3)]).cpu().numpy().reshape(2, 2, 3, 3),
                               2 * _PAF_KAT, atol=1e-3)

    gen = torch.Generator().manual_seed(5)
    big = torch.rand((4, 9, 13, 2), generator=gen) * torch.tensor([300.0, 260.0]) - 20.0
    big[torch.rand((4, 9, 13), generator=gen) < 0.15] = float("nan")
    edges = [(i, i + 1) for i in range(12)]
    hw = (250, 282)  # not a multiple of the stride: grid = ceil(size / stride)
    cm = generate_multiconfmaps(big.cuda(), hw, sigma=2.0, output_stride=4).cpu()
    torch.testing.assert_close(cm, O.make_multiconfmaps(big, hw, 2.0, 4), rtol=0, atol=2e-6)
    pf = generate_pafs(big.cuda(), hw, sigma=20.0, output_stride=8, edge_inds=edges).cpu()
    ref = torch.stack([O.make_pafs_sample(big[b], edges, hw, 20.0, 8) for b in range(4)])
    torch.testing.assert_close(pf, ref, rtol=0, atol=1e-5)
    # centroid form (B, I, 2) -> one channel
    cen = generate_multiconfmaps(big[:, :, 0].cuda(), hw, sigma=2.0, output_stride=2).cpu()
    torch.testing.assert_close(cen, O.make_multiconfmaps(big[:, :, :1], hw, 2.0, 2), rtol=0, atol=2e-6)


def test_multiclass_topdown_training_matches_autograd():
    """multi_class_topdown: MSE on the confidence maps + the reference's CrossEntropyLoss on the class-vector
    head's softmax output (lightning_modules.py:2655-2677), backward through softmax, the FC stack (row GEMMs),
    the global max pool and the encoder; vs autograd over the oracle."""
    from sleap_nn_amd.architectures.model import Model
    from sleap_nn_amd.training.module import TrainingModule

    bb = {"in_channels": 1, "kernel_size": 3, "filters": 8, "filters_rate": 1.5, "max_stride": 16, "stem_stride": None, "middle_block": True,
          "up_interpolate": True, "stacks": 1, "convs_per_block": 2, "output_stride": 2}
    heads = {"confmaps": {"part_names": ["A", "B"], "anchor_part": "A", "sigma": 1.5, "output_stride": 2, "loss_weight": 1.0},
             "class_vectors": {"classes": ["f", "m", "x"], "num_fc_layers": 2, "num_fc_units": 32, "global_pool": True, "output_stride": 16, "loss_weight": 0.3}}
    mt = "multi_class_topdown"
    g = torch.Generator().manual_seed(19)
    m = Model("unet", bb, heads, mt)
    sd = {}
    for k, shape in m.param_shapes.items():
        fan = int(np.prod(shape[1:])) if len(shape) > 1 else 1
        sd[k] = (torch.rand(shape, generator=g) * 2 - 1) * (1.5 / np.sqrt(fan) if len(shape) > 1 else 0.1)
    m.load_state_dict(sd)
    B = 5
    img = torch.randint(0, 256, (B, 1, 64, 48), dtype=torch.uint8, generator=g)
    ref_out = O.model_forward(sd, bb, heads, mt, img)
    targets = {"CenteredInstanceConfmapsHead": torch.rand(ref_out["CenteredInstanceConfmapsHead"].shape, generator=g) * 0.5,
               "ClassVectorsHead": torch.nn.functional.one_hot(torch.randint(0, 3, (B,), generator=g), 3).float()}
    lw = [1.0, 0.3]
    tm = TrainingModule(m, DEV, loss_weights=lw)
    losses, ref_grads = O.training_step(sd, bb, heads, mt, img, targets, lw)
    loss = tm.forward_backward(img.to(DEV), {k: v.to(DEV) for k, v in targets.items()})
    torch.cuda.synchronize()
    got = loss.cpu().numpy()
    np.testing.assert_allclose(got, np.array(losses), rtol=2e-5, atol=1e-6)
    _check_grads(tm, ref_grads, rtol=2e-4)


@pytest.mark.parametrize("conv_wino,floor", [(1, 6e-4), (0, 1e-4)])
def test_backward_cfg3_network_with_interior_tiles(conv_wino, floor):
    """Backward parity of the benched network (cfg3, 7.8 M parameters) at a size whose feature maps have interior tiles in
    every kernel (256x320, B=2; the cases above use small nets).  The yardstick is the float64 oracle: at this depth fp32
    autograd itself is up to ~6e-4 of a tensor's scale away from it (torch-CPU fp32 vs the same oracle in float64) -- not
    through rounding of the sums but through ReLU masks: an activation within rounding distance of zero is "on" in one
    evaluation and "off" in the other, and each flipped pixel moves the gradient by a whole term.  Every HIP gradient must be
    within `floor` of the float64 one or within twice torch's own fp32 error for that tensor.  With the direct 9-tap kernels
    everywhere (conv_wino = 0) the floor is 1e-4 (measured worst 1.0e-4; torch 5.8e-5); the default Winograd F(2,3) forward is
    ~5x further from the exact activations (1e-6 vs 2e-7 relative, both inside the 1e-4 forward bar), flips more masks, and its
    worst weight gradient sits 4.2e-4 from the float64 one -- the gradient of the function the forward actually computed, not
    an arithmetic defect: switching only the data-gradient convs to direct kernels (dgrad_wino = 0) changes no digit of it."""
    import bench

    bb, heads, mt = dict(bench.CFG3_BB), {k: dict(v) for k, v in bench.CFG3_HEADS.items()}, "bottomup"
    sd, img, targets, lw, tm = _setup(bb, heads, mt, (256, 320), 2, seed=3)
    tm.model.set_option("conv_wino", conv_wino)
    ref_losses, g32 = O.training_step(sd, bb, heads, mt, img, targets, lw)
    _, g64 = O.training_step({k: v.double() for k, v in sd.items()}, bb, heads, mt, img, {k: v.double() for k, v in targets.items()}, lw)
    loss = tm.forward_backward(img, targets).cpu().numpy()
    assert np.allclose(loss, np.array(ref_losses, dtype=np.float32), rtol=1e-5, atol=1e-6)
    got = tm.named_grads()
    worst = []
    for k, r in g64.items():
        scale = max(float(r.abs().max()), 1e-30)
        e_hip = float((got[k].double() - r).abs().max()) / scale
        e_ref = float((g32[k].double() - r).abs().max()) / scale
        worst.append((e_hip, e_ref, k))
    worst.sort(reverse=True)
    print(f"cfg3 256x320 backward vs float64 oracle (conv_wino={conv_wino}): worst (hip err, torch-fp32 err, tensor)", worst[:4])
    for e_hip, e_ref, k in worst:
        assert e_hip <= max(floor, 2.0 * e_ref), (k, e_hip, e_ref)


@pytest.mark.parametrize("seed", [0, 7])
def test_backward_randomised_shapes(seed):
    """A few draws of the randomised sweep (tools/stress_backward.py): awkward channel counts, odd tile counts, both model types."""
    rng = np.random.default_rng(seed)
    done = 0
    while done < 3:
        down = int(rng.integers(2, 5))
        os_ = int(2 ** rng.integers(0, min(3, down)))
        bb = {"in_channels": int(rng.choice([1, 3])), "kernel_size": 3, "filters": int(rng.choice([4, 8, 12, 16, 20, 24, 32])), "filters_rate": float(rng.choice([1.5, 2.0])),
              "max_stride": 2**down, "stem_stride": None, "middle_block": True, "up_interpolate": True, "stacks": 1, "convs_per_block": 2, "output_stride": os_}
        names = [f"n{i}" for i in range(int(rng.integers(2, 5)))]
        mt = str(rng.choice(["single_instance", "bottomup"]))
        heads = {"confmaps": {"part_names": names, "output_stride": os_, "loss_weight": 1.0}}
        if mt == "bottomup":
            heads["pafs"] = {"edges": [[names[i], names[i + 1]] for i in range(len(names) - 1)], "output_stride": min(2**down, os_ * 2), "loss_weight": 0.5}
        mult = 2**down
        B = int(rng.integers(1, 4))
        hw = (mult * int(rng.integers(1, 7)), mult * int(rng.integers(1, 7)))
        try:
            sd, img, targets, lw, tm = _setup(bb, heads, mt, hw, B, seed=int(rng.integers(1 << 30)))
        except ValueError:  # a PAF stride the decoder does not produce: not a valid reference config either
            continue
        ref_losses, ref_grads = O.training_step(sd, bb, heads, mt, img, targets, lw)
        loss = tm.forward_backward(img, targets).cpu().numpy()
        assert np.allclose(loss, np.array(ref_losses, dtype=np.float32), rtol=1e-5, atol=1e-6), (bb, heads, hw, B)
        _check_grads(tm, ref_grads)
        done += 1


@pytest.mark.parametrize("case", ["cpb3", "cpb1"])
def test_backward_with_other_convs_per_block(case):
    """convs_per_block 3 (three convs per encoder block, two expand convs in the middle block) and 1 (no middle block, rate 1: the only
    one-conv UNet the reference runs): the backward plan walks the same op list, in which the decoder blocks keep two refine convs whatever
    the key says (unet.py:203-216 of the reference).  Losses and every gradient against the oracle's autograd step."""
    bb, heads, mt = _cfg(16, 16, 2)
    if case == "cpb3":
        bb.update(convs_per_block=3)
        hw, B = (48, 80), 2
    else:
        bb.update(convs_per_block=1, middle_block=False, filters_rate=1, in_channels=3)
        hw, B = (48, 112), 3
    sd, img, targets, lw, tm = _setup(bb, heads, mt, hw, B, seed=23)
    n_refine = sum(1 for k in sd if "_refine_conv" in k and k.endswith(".weight"))
    assert n_refine == 2 * 3 and not any("_refine_conv2" in k for k in sd)  # three decoder blocks (stride 16 -> 2), two refine convs each
    assert any("_conv2.weight" in k for k in sd) == (case == "cpb3")
    ref_losses, ref_grads = O.training_step(sd, bb, heads, mt, img, targets, lw)
    loss = tm.forward_backward(img, targets).cpu().numpy()
    assert np.allclose(loss, np.array(ref_losses, dtype=np.float32), rtol=1e-5, atol=1e-6), (loss, ref_losses)
    worst = _check_grads(tm, ref_grads)
    print(f"convs_per_block {case}: loss {loss.tolist()} vs {ref_losses}, worst gradient error {worst:.2e} of its tensor's scale")
    g1 = tm.grads.clone()
    tm.forward_backward(img, targets)
    assert torch.equal(g1, tm.grads)


def test_eval_train_round_trip_keeps_trained_weights():
    """After optimizer steps the live parameters exist only in the TrainingModule's device arena.  Wrapping the model in a
    HipBackend for validation switches it to the fused program (handle rebuilt) and train() switches back: both
    recompiles must pick the arena's CURRENT values up, not the initial host copy."""
    from sleap_nn_amd.inference.backends import HipBackend

    bb, heads, mt = _cfg(8, 8, 2)
    sd, img, targets, lw, tm = _setup(bb, heads, mt, (48, 64), 2, seed=11, lr=1e-2)
    for _ in range(3):
        tm.training_step({"image": img, **targets})
    trained = tm.state_dict()
    assert any(not torch.equal(trained[k], sd[k]) for k in sd)
    ref = O.model_forward({k: v.clone() for k, v in trained.items()}, bb, heads, mt, img)
    val = HipBackend(tm.model, DEV)(img)  # eval(): fused program, new handle
    for k, v in ref.items():
        assert (val[k].cpu() - v).abs().max().item() <= 1e-4, k
    tm.model.train(True)  # back to the training program: another new handle
    ref_losses, ref_grads = O.training_step(trained, bb, heads, mt, img, targets, lw)
    loss = tm.forward_backward(img, targets).cpu().numpy()
    assert np.allclose(loss, np.array(ref_losses, dtype=np.float32), rtol=1e-5, atol=1e-6)
    _check_grads(tm, ref_grads)


def test_training_step_matches_reference_fixture_with_negative_weighting_and_ohkm():
    """losses.npz "step": loss and every parameter gradient of ONE training step of the reference ``Model`` itself
    (negative-sample-weighted MSE + OHKM per head, loss weights 1.0 / 0.6), reproduced by ph_model_backward.  Also the
    val stage (unweighted) and the is_negative-absent path against the oracle."""
    import json

    from sleap_nn_amd.architectures.model import Model
    from sleap_nn_amd.training.module import OHKMConfig, TrainingModule
    from tests import _golden as G

    z = G.load("losses.npz")
    cfg = json.loads(str(z["step/config_json"]))
    sd = {k[len("step/w/"):]: torch.from_numpy(z[k]) for k in z.files if k.startswith("step/w/")}
    tg = {k[len("step/target/"):]: torch.from_numpy(z[k]) for k in z.files if k.startswith("step/target/")}
    img, neg = torch.from_numpy(z["step/image"]), torch.from_numpy(z["step/is_negative"])
    m = Model("unet", cfg["backbone"], cfg["heads"], cfg["model_type"])
    m.load_state_dict(sd)
    ok = cfg["ohkm"]
    tm = TrainingModule(m, DEV, loss_weights=cfg["loss_weights"], negative_loss_weight=cfg["negative_loss_weight"],
                        ohkm=OHKMConfig(True, ok["hard_to_easy_ratio"], ok["min_hard_keypoints"], None if ok["max_hard_keypoints"] < 0 else ok["max_hard_keypoints"], ok["loss_scale"]))
    loss = tm.forward_backward(img, tg, is_negative=neg).cpu().numpy()
    assert np.allclose(loss, z["step/losses"], rtol=2e-5), (loss, z["step/losses"])
    _check_grads(tm, {k[len("step/g/"):]: torch.from_numpy(z[k]) for k in z.files if k.startswith("step/g/")})
    okd = dict(hard_to_easy_ratio=ok["hard_to_easy_ratio"], min_hard_keypoints=ok["min_hard_keypoints"], max_hard_keypoints=None, loss_scale=ok["loss_scale"])
    for kw in (dict(is_negative=neg, stage="val"), dict(is_negative=None, stage="train")):
        ref_l, ref_g = O.training_step(sd, cfg["backbone"], cfg["heads"], cfg["model_type"], img, tg, cfg["loss_weights"], ohkm=okd,
                                       negative_loss_weight=cfg["negative_loss_weight"], **kw)
        got = tm.forward_backward(img, tg, **kw).cpu().numpy()
        assert np.allclose(got, np.array(ref_l, dtype=np.float32), rtol=2e-5), kw
        _check_grads(tm, ref_g)


def test_lr_schedule_drives_the_optimizer():
    """TrainingModule(lr_scheduler=...): ``lr`` follows the reference's schedule, one step per epoch (schedulers.npz holds the
    learning rates the reference's schedulers produce); the Adam update of the next step uses it."""
    from tests import _golden as G

    z = G.load("schedulers.npz")
    bb, heads, mt = _cfg(8, 8, 2)
    sd, img, targets, lw, tm = _setup(bb, heads, mt, (32, 32), 1, seed=5, lr=1e-3,
                                      lr_scheduler={"cosine_annealing_warmup": {"warmup_epochs": 4, "max_epochs": 25, "warmup_start_lr": 1e-5, "eta_min": 1e-6}})
    lrs = [tm.lr]
    for _ in range(6):
        lrs.append(tm.on_epoch_end(val_loss=1.0))
    assert np.allclose(lrs, z["cosine"][:7], rtol=1e-12, atol=0)
    before = tm.params.clone()
    tm.training_step({"image": img, **targets})
    step = (tm.params - before).abs().max().item()
    assert 0.5 * tm.lr <= step <= 1.5 * tm.lr  # first Adam step moves every touched weight by ~lr
    tm2 = _setup(bb, heads, mt, (32, 32), 1, seed=5, lr=1e-3, lr_scheduler="step_lr")[-1]
    for e in range(10):
        tm2.on_epoch_end()
    assert abs(tm2.lr - 1e-4) < 1e-12  # StepLR defaults: step_size 10, gamma 0.1


@pytest.mark.parametrize("case", ["tiny_trans", "wide_trans_odd"])
def test_backward_with_transposed_conv_decoder(case):
    """up_interpolate=False (ConvTranspose2d(k3, s2, p1, op1) + ReLU up-sampling, encoder_decoder.py:439-461): forward through
    the four output-phase GEMMs, weight gradient by nine stride-2-gathered row GEMMs, data gradient as a 3x3 stride-2 conv --
    loss and every parameter gradient vs autograd over the oracle."""
    if case == "tiny_trans":
        bb, heads, mt = _cfg(8, 8, 2)
        bb["filters_rate"] = 1.5
        hw, B = (48, 80), 2
    else:
        bb, heads, mt = _cfg(24, 16, 4, n_nodes=4)
        hw, B = (96, 112), 3
    bb["up_interpolate"] = False
    sd, img, targets, lw, tm = _setup(bb, heads, mt, hw, B, seed=23)
    assert any("trans_conv" in k for k in sd)
    ref_losses, ref_grads = O.training_step(sd, bb, heads, mt, img, targets, lw)
    loss = tm.forward_backward(img, targets).cpu().numpy()
    assert np.allclose(loss, np.array(ref_losses, dtype=np.float32), rtol=1e-5, atol=1e-6)
    _check_grads(tm, ref_grads)


def test_fine_tuning_the_reference_bottomup_fixture_checkpoint():
    """The reference's own bottom-up fixture checkpoint (minimal_instance_bottomup, up_interpolate: false) takes training
    steps: gradients of the first step vs autograd over the oracle on its golden frames, then three Adam steps lower the loss."""
    from sleap_nn_amd.architectures.model import Model
    from sleap_nn_amd.training.module import TrainingModule
    from tests import _golden as G

    z = G.load("ckpt_bottomup.npz")
    cfg = G.config(z)
    bb, heads, mt = cfg["backbone"], cfg["heads"], cfg["model_type"]
    sd = G.weights(z)
    img = torch.from_numpy(z["image"]).squeeze(1)[:, :, :192, :256].contiguous()
    tg = {k[4:]: torch.from_numpy(z[k])[:, :, : 192 // (2 if "Confmaps" in k else 4), : 256 // (2 if "Confmaps" in k else 4)].contiguous() * 0.9 + 0.01 for k in z.files if k.startswith("out/")}
    m = Model("unet", bb, heads, mt)
    m.load_state_dict(sd)
    lw = [h.loss_weight for h in m.heads]
    tm = TrainingModule(m, DEV, lr=1e-4, loss_weights=lw)
    ref_losses, ref_grads = O.training_step(sd, bb, heads, mt, img, tg, lw)
    first = tm.forward_backward(img, tg).cpu().numpy()
    assert np.allclose(first, np.array(ref_losses, dtype=np.float32), rtol=1e-5, atol=1e-7)
    _check_grads(tm, ref_grads)
    losses = [float(tm.training_step({"image": img, **tg})[0]) for _ in range(4)]
    assert losses[-1] < losses[0]


@pytest.mark.parametrize("case", ["k5_bilinear", "k5_transposed_rgb", "k7_small", "stem_block", "stem_block_wide"])
def test_backward_of_wide_kernels_and_stem_blocks(case):
    """kernel_size 5 / 7 and StemBlock UNets train (VERDICT r2 "Missing 1"; encoder_decoder.py:38-141,144-225, unet.py:230-253): the k x k
    weight gradient is k^2 row-wgrad GEMMs (one per tap), the data gradient the k^2-tap row GEMM on the flipped, in/out-swapped weights
    (accumulating into skip tensors), the first k x k conv's weight gradient an im2col + one row-wgrad GEMM.  Loss and every parameter
    gradient vs autograd over the oracle, then an Adam step that lowers the loss."""
    if case == "k5_bilinear":
        bb, heads, mt = _cfg(8, 8, 2)
        bb["kernel_size"] = 5
        hw, B = (48, 64), 2
    elif case == "k5_transposed_rgb":
        bb, heads, mt = _cfg(12, 8, 2, in_ch=3, bottomup=False)
        bb["kernel_size"] = 5
        bb["up_interpolate"] = False
        hw, B = (40, 56), 3
    elif case == "k7_small":
        bb, heads, mt = _cfg(8, 4, 1, bottomup=False)
        bb["kernel_size"] = 7
        hw, B = (32, 40), 2
    elif case == "stem_block":
        bb, heads, mt = _cfg(8, 16, 4)
        bb["stem_stride"] = 2
        hw, B = (64, 96), 2
    else:  # wider channels: N tiles of 64 in the 7x7 data-gradient GEMMs, 3x3 layers on the Winograd kernels next to them
        bb, heads, mt = _cfg(24, 16, 2, n_nodes=4)
        bb["stem_stride"] = 2
        hw, B = (64, 64), 3
    sd, img, targets, lw, tm = _setup(bb, heads, mt, hw, B, seed=31)
    ref_losses, ref_grads = O.training_step(sd, bb, heads, mt, img, targets, lw)
    loss = tm.forward_backward(img, targets).cpu().numpy()
    assert np.allclose(loss, np.array(ref_losses, dtype=np.float32), rtol=1e-5, atol=1e-6)
    worst = _check_grads(tm, ref_grads)
    assert worst <= 1e-4
    batch = {"image": img, **targets}
    first = float(tm.training_step(batch)[0])
    for _ in range(3):
        last = float(tm.training_step(batch)[0])
    assert np.isfinite(last) and last < first


def test_winograd_weight_gradients_against_the_float64_oracle_per_tensor():
    """the end-to-end Adam bound of the default weight-gradient path (wgrad_wino = 1) is loose by design; this pins
    wgrad_wino_kernel / wgrad16_wino_kernel directly: every parameter gradient of one step against the FLOAT64 oracle, per tensor
    max error / tensor scale, for the Winograd-domain kernels and for the direct kernels of the same handle (both ~1e-6: fp32 rounding)."""
    bb, heads, mt = _cfg(16, 16, 4, n_nodes=4)
    hw, B = (96, 128), 2
    sd, img, targets, lw, tm = _setup(bb, heads, mt, hw, B, seed=37)
    sd64 = {k: v.double() for k, v in sd.items()}
    _, ref64 = O.training_step(sd64, bb, heads, mt, img, {k: v.double() for k, v in targets.items()}, lw)
    worst = {}
    for wino in (1, 0):
        tm.model.set_option("wgrad_wino", wino)
        tm.forward_backward(img, targets)
        got = tm.named_grads()
        w = 0.0
        for k, r in ref64.items():
            scale = max(float(r.abs().max()), 1e-30)
            w = max(w, float((got[k].double() - r).abs().max()) / scale)
        worst[wino] = w
    assert worst[1] <= 5e-6 and worst[0] <= 5e-6, worst


@pytest.mark.parametrize("rows,n,k", [(10007, 96, 48), (4133, 384, 96), (4133, 96, 384), (2050, 768, 192), (1000, 256, 128), (777, 48, 16)])
def test_row_weight_gradient_gemm_tile_plans_against_a_float64_sum(rows, n, k):
    """The row weight-gradient GEMM dW[n][k] = sum_m dY[m][n] X[m][k] in each of its tile plans: 128-wide k tiles, 96-wide k tiles (a k operand
    that is a multiple of 96 but not of 128: ConvNeXt widths 96 / 192), the operands exchanged (the n operand is the one like that), a partial last
    chunk of rows (rows % 32 != 0: the general fetch path next to the descriptor one).  64 sampled entries against a float64 host sum, relative to the
    largest of them; fp32 accumulation over up to 10 007 rows of values in [-0.5, 0.5): measured <= 4e-7."""
    import ctypes as C
    from sleap_nn_amd import _lib as L

    ms, err = C.c_float(), C.c_float()
    L.check(L.lib().ph_debug_row_wgrad_bench(rows, n, k, 1, C.byref(ms), C.byref(err)))
    assert err.value < 2e-6, err.value
