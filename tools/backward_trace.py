"""Record of ph_model_backward over a fixed list of tiny training programs: the check of a change to the backward's host code (csrc/backward.hip, csrc/train.hip) that must not
move a launch, an argument or a byte.  The sibling of tools/forward_trace.py, whose config builders and ``make`` / ``image`` helpers it reuses.

    python tools/backward_trace.py OUT.jsonl

One JSON line per case: its name, ``ph_model_backward_workspace_bytes``, the pad-vector offset and length (Swin programs), the gradient arena's bucket split,
``last_backward_kernels()``, ``last_backward_routes()`` and a SHA-256 of the loss tensor, of the gradient arena and of the whole gradient workspace.  Arena and workspace are zeroed before the recorded
step, which follows one unrecorded step that sizes the buffers.  Cases run with profiling record the SET of ops whose ``op_ms_first`` is non-zero (not the times).  Run it on
a build of the commit before the change and on a build of the change, on the same device: the backward is deterministic by contract (fixed-order reductions, no float
atomics), so the two files are byte-identical unless a route, an argument or the plan changed.  Under ``rocprofv3 --kernel-trace -- python tools/backward_trace.py ...`` the
ordered kernel list of the two runs shows a duplicated or dropped launch that happens to leave the same bytes.

Cases (batch 2, 64 x 96; the UNets also 72 x 104, whose pooled maps are odd-sized): the seven UNet variants with bottom-up heads, ``wino4`` on and off; on the bilinear and
the transposed variant each backward option on its own (``mask_fold``, ``wgrad_wino``, ``wgrad_rows`` 1 / 2, ``dgrad_wino``, ``pool_peephole``, OHKM, negative frames); a
class-vector top-down model; a segmentation model; ConvNeXt (``fuse_gelu_bwd`` x ``fuse_gelu_fwd``); Swin without and with branch scales; ConvNeXtV2, unfrozen and frozen;
the two-bucket schedule (a bucket event, a one-rank communicator); and the calls ph_model_backward refuses (return code and error text)."""
import ctypes as C
import hashlib
import json
import sys
import time

sys.path.insert(0, ".")
import torch

from sleap_nn_amd import _lib as L
from sleap_nn_amd.training.module import OHKMConfig, TrainingModule
from sleap_nn_amd.training.segmentation import SegmentationTrainingModule
from tools.forward_trace import DEV, convnext_cfg, convnextv2_cfg, image, make, swin_cfg, unet_cfg

OUT = None
N_CASES = 0
BACKWARD_OPTIONS = (("mask_fold", 0, 1), ("wgrad_wino", 0, 1), ("wgrad_rows", 1, 0), ("wgrad_rows", 2, 0), ("dgrad_wino", 0, 1), ("pool_peephole", 0, 1))  # (name, value, default)


def sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def write(row):
    global N_CASES
    OUT.write(json.dumps(row, sort_keys=True) + "\n")
    OUT.flush()
    N_CASES += 1


def targets_for(tm, img, seed):
    """Seeded targets in the shapes the module's heads take: one-hot rows for a class-vector head, a binary map for a BCE + Dice head and for the weight-mask channel
    of the offsets, uniform [0, 0.5) elsewhere."""
    m = tm.model
    out = m.forward(tm.model.adapt_channels(img, 0)[0] if getattr(tm, "_pretrained", False) else img)
    g = torch.Generator().manual_seed(seed)
    tg = {}
    for i, h in enumerate(m.heads):
        shape = tm._target_shape(i, tuple(out[h.name].shape))
        t = torch.rand(shape, generator=g) * 0.5
        if len(shape) == 2:
            t = torch.nn.functional.one_hot(torch.randint(0, shape[1], (shape[0],), generator=g), shape[1]).float()
        elif getattr(h, "loss_function", None) == "bce_dice":
            t = (t > 0.25).float()
        elif getattr(h, "loss_function", None) == "smooth_l1":
            t[:, -1] = (t[:, -1] > 0.25).float()
        tg[h.name] = t.to(DEV)
    return tg


def record(name, tm, img, targets, is_negative=None, scales=None, profile=False):
    m = tm.model
    lib = L.lib()
    B, _, H, W = img.shape

    def step():
        if scales is not None:
            tm.set_branch_scales(scales)
        tm.forward_backward(img, targets, is_negative)
        torch.cuda.synchronize()

    step()  # (sizes the buffers for this setting)
    tm.grads.zero_()
    tm._grad_ws.zero_()
    if profile:
        m.set_profiling(True)
    step()
    need = int(L.check(lib.ph_model_backward_workspace_bytes(m._handle, B, H, W)))
    row = {"case": name, "workspace_bytes": need, "bucket_split": int(L.check(lib.ph_model_grad_bucket_split(m._handle))), "kernels": m.last_backward_kernels(),
           "routes": m.last_backward_routes(), "sha256": {"loss": sha(tm._loss), "grads": sha(tm.grads), "grad_workspace": sha(tm._grad_ws[:need])}}
    if any(o.kind == L.OP_WINDOW_ATTN for o in m.ops):
        n = C.c_int32()
        row["pad_vector"] = [int(L.check(lib.ph_model_backward_pad_vector(m._handle, B, H, W, C.byref(n)))), n.value]
    if profile:
        n = len(m.ops)
        op_ms, first, lm = (C.c_double * n)(), (C.c_double * n)(), C.c_double()
        L.check(lib.ph_model_backward_profile_read(m._handle, op_ms, first, n, C.byref(lm)))
        row["ops_with_first_part"] = [i for i in range(n) if first[i] != 0.0]
        m.set_profiling(False)
    write(row)


def unet_cases():
    for variant in ("bilinear", "transposed", "cpb1", "cpb3", "stem", "k5", "filters24"):
        for hw in ((64, 96), (72, 104)):
            bb, heads, mt = unet_cfg(variant)
            img = image(2, 1, hw, hw[1])
            for wino4 in (True, False):
                tm = TrainingModule(make("unet", bb, heads, mt, hw[0]), DEV, wino4=wino4)
                tg = targets_for(tm, img, hw[0] + 1)
                tag = f"unet {variant} {hw[0]}x{hw[1]} wino4={int(wino4)}"
                record(f"{tag} defaults", tm, img, tg, profile=(wino4 and hw[0] == 64 and variant in ("bilinear", "transposed", "k5")))
                if not (wino4 and variant in ("bilinear", "transposed")):
                    continue
                for key, value, default in BACKWARD_OPTIONS:
                    tm.model.set_option(key, value)
                    record(f"{tag} {key}={value}", tm, img, tg)
                    tm.model.set_option(key, default)
                tm.ohkm = OHKMConfig(online_mining=True, hard_to_easy_ratio=1.05, min_hard_keypoints=2, loss_scale=5.0)
                record(f"{tag} ohkm", tm, img, tg)
                tm.ohkm = OHKMConfig()
                tm.negative_loss_weight = 0.5
                record(f"{tag} is_negative, negative_loss_weight=0.5", tm, img, tg, is_negative=torch.tensor([True, False]))
                tm.negative_loss_weight = 1.0


def other_backbone_cases():
    hw = (64, 96)
    bb = {"in_channels": 1, "kernel_size": 3, "filters": 8, "filters_rate": 1.5, "max_stride": 16, "stem_stride": None, "middle_block": True, "up_interpolate": True, "stacks": 1,
          "convs_per_block": 2, "output_stride": 2}
    heads = {"confmaps": {"part_names": ["A", "B"], "anchor_part": "A", "sigma": 1.5, "output_stride": 2, "loss_weight": 1.0},
             "class_vectors": {"classes": ["f", "m", "x"], "num_fc_layers": 2, "num_fc_units": 32, "global_pool": True, "output_stride": 16, "loss_weight": 0.3}}
    tm = TrainingModule(make("unet", bb, heads, "multi_class_topdown", 19), DEV)
    img = image(2, 1, hw, 23)
    record("class-vector top-down unet", tm, img, targets_for(tm, img, 24), profile=True)

    bb = {"in_channels": 1, "kernel_size": 3, "filters": 16, "filters_rate": 2, "max_stride": 16, "stem_stride": None, "middle_block": True, "up_interpolate": True, "stacks": 1,
          "convs_per_block": 2, "output_stride": 2}
    heads = {"segmentation": {"output_stride": 2, "loss_weight": 1.0}, "center": {"sigma": 4.0, "output_stride": 2, "loss_weight": 1.0}, "offsets": {"output_stride": 2, "loss_weight": 0.1}}
    tm = SegmentationTrainingModule(make("unet", bb, heads, "bottomup_segmentation", 29), DEV)
    img = image(2, 1, hw, 31)
    record("bottom-up segmentation unet (BCE + Dice, centre MSE, masked smooth-L1)", tm, img, targets_for(tm, img, 32))

    bb, heads, mt = convnext_cfg([24, 40, 72, 136])
    tm = TrainingModule(make("convnext", bb, heads, mt, 4), DEV)
    img = image(2, 1, hw, 19)
    tg = targets_for(tm, img, 20)
    for bwd in (1, 0):
        for fwd in (1, 0):
            tm.model.set_option("fuse_gelu_bwd", bwd)
            tm.model.set_option("fuse_gelu_fwd", fwd)
            record(f"convnext 24 fuse_gelu_bwd={bwd} fuse_gelu_fwd={fwd}", tm, img, tg, profile=(bwd == 1 and fwd == 1))

    bb, heads, mt = swin_cfg()
    tm = TrainingModule(make("swint", bb, heads, mt, 7), DEV, swint_training=True, stochastic_depth_prob=0.0)
    img = image(2, 1, hw, 11)
    tg = targets_for(tm, img, 12)
    record("swint small, no branch scales", tm, img, tg, profile=True)
    n = tm.model.residual_branches()
    scales = 0.5 + torch.arange(2 * n, dtype=torch.float32).reshape(n, 2) / (2 * n)
    scales[1, 0] = 0.0
    scales[n - 1, 1] = 0.0
    record("swint small, fixed branch scales with zeros", tm, img, tg, scales=scales)

    bb, heads, mt = convnextv2_cfg()
    img = image(2, 3, hw, 13)
    for freeze in (False, True):
        tm = TrainingModule(make("pretrained", bb, heads, mt, 9), DEV, pretrained_training=True, freeze_encoder=freeze)
        record(f"convnextv2 tiny freeze_encoder={int(freeze)}", tm, img, targets_for(tm, img, 14), profile=True)


def bucket_cases():
    """The two-bucket schedule inside the backward (tests/test_gpu_training.py::test_native_rccl_exchange_runs_the_two_bucket_schedule_inside_the_backward)."""
    from sleap_nn_amd.parallel import Communicator

    hw = (64, 96)
    bb, heads, mt = unet_cfg("bilinear")
    cbb, cheads, cmt = convnextv2_cfg()
    for name, build, channels in (("unet bilinear", lambda: TrainingModule(make("unet", bb, heads, mt, 3), DEV), 1),
                                  ("convnextv2 tiny frozen (split op in the frozen prefix)",
                                   lambda: TrainingModule(make("pretrained", cbb, cheads, cmt, 9), DEV, pretrained_training=True, freeze_encoder=True), 3)):
        tm = build()
        img = image(2, channels, hw, 17)
        tm._bucket_event = torch.cuda.Event()  # (every step hands it to ph_model_set_bucket_event)
        tm._bucket_event.record()
        record(f"bucket event: {name}", tm, img, targets_for(tm, img, 18), profile=True)
        tm._bucket_event.synchronize()
        tm.close()
    if not Communicator.available():
        write({"case": "one-rank communicator: unet bilinear", "skipped": "librccl could not be opened (Communicator.available() is false)"})
        return
    tm = TrainingModule(make("unet", bb, heads, mt, 3), DEV)
    img = image(2, 1, hw, 17)
    tm._comm, tm._comm_stream = Communicator.create(torch.device(DEV)), torch.cuda.Stream(DEV)
    record("one-rank communicator: unet bilinear", tm, img, targets_for(tm, img, 18))
    tm.close()


def refusal(name, tm, img, prepare, short_by=0):
    """One ph_model_backward call that must be refused before any launch: ``prepare(model)`` twists the handle, a forward follows, then the call as TrainingModule makes it."""
    m = tm.model
    lib = L.lib()
    tg = targets_for(tm, img, 5)
    B, Cin, H, W = img.shape
    need = int(lib.ph_model_backward_workspace_bytes(m._handle, B, H, W))  # (of the untwisted program)
    ws = torch.zeros(max(need, 1 << 20), dtype=torch.uint8, device=DEV)
    prepare(m)
    out = m.forward(img)
    outs = [out[h.name].contiguous() for h in m.heads]
    tgs = [tg[h.name] for h in m.heads]
    optr = (C.c_void_p * len(outs))(*[o.data_ptr() for o in outs])
    tptr = (C.c_void_p * len(tgs))(*[t.data_ptr() for t in tgs])
    lw = (C.c_float * len(outs))(*([1.0] * len(outs)))
    torch.cuda.synchronize()
    rc = lib.ph_model_backward(m._handle, C.c_void_p(img.data_ptr()), 0, B, Cin, H, W, C.c_void_p(m._workspace.data_ptr()), C.c_void_p(ws.data_ptr()),
                               (need - short_by) if short_by else ws.numel(), optr, tptr, lw, None, 0, 2.0, 2, -1, 5.0, C.c_void_p(tm._loss.data_ptr()), C.c_void_p(tm.grads.data_ptr()),
                               L.current_stream_ptr())
    torch.cuda.synchronize()
    write({"case": f"refusal: {name}", "rc": int(rc), "error": lib.ph_last_error().decode() if rc != 0 else ""})


def refusal_cases():
    hw = (64, 96)
    bb, heads, mt = unet_cfg("bilinear")
    img = image(2, 1, hw, 41)
    new = lambda: TrainingModule(make("unet", bb, heads, mt, 3), DEV)  # noqa: E731
    refusal("forward of the fused inference handle", new(), img, lambda m: m.eval())
    refusal("forward of the fused inference handle, every activation kept", new(), img, lambda m: (m.eval(), m.set_option("workspace_reuse", 0)))
    refusal("fp16 forward", new(), img, lambda m: m.set_option("conv_precision", 2))
    refusal("workspace_reuse 1", new(), img, lambda m: m.set_option("workspace_reuse", 1))
    refusal("gradient workspace one byte short", new(), img, lambda m: None, short_by=1)
    cbb, cheads, cmt = convnextv2_cfg()
    tm = TrainingModule(make("pretrained", cbb, cheads, cmt, 9), DEV, pretrained_training=True)
    refusal("convnextv2 handle with pretrained_train 0", tm, image(2, 3, hw, 13), lambda m: m.set_option("pretrained_train", 0))


def main():
    global OUT
    t0 = time.time()
    OUT = open(sys.argv[1], "w")
    with torch.cuda.device(torch.device(DEV)):
        unet_cases()
        other_backbone_cases()
        bucket_cases()
        refusal_cases()
    OUT.close()
    print(f"{N_CASES} cases in {time.time() - t0:.1f} s -> {sys.argv[1]}")


if __name__ == "__main__":
    main()
