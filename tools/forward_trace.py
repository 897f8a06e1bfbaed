"""Routing and output record of ph_model_forward over a fixed list of tiny programs: the check of a change to the router (csrc/forward.hip, csrc/plan.hip) that must not
move a launch or a byte.

    python tools/forward_trace.py OUT.jsonl

One JSON line per case: its name, ``last_kernels()``, the rows of ``last_ranges()`` and a SHA-256 of every output tensor's bytes.  Run it on a build of the commit
before the change and on a build of the change, on the same device: every kernel is deterministic and batch-invariant (tests/test_gpu_*), so the two files are
byte-identical unless a route or an argument changed.  The workspace is zeroed before each recorded forward, so a range that is read without having been written shows
the same bytes in both runs.

Cases: what tests/test_gpu_plan_hazards.py::_sweep walks (seven UNet variants at 64 x 96 and 72 x 104, two ConvNeXt widths; exact / split / fp16; the test's routing
pins; defaults, each fusion option off in turn, the op-by-op program on shared slots), each with ``workspace_reuse`` on and off, plus the same models without pins,
a Swin program (fp32 and ``swint_f16``), a ConvNeXtV2 program (``grn_fuse`` 0 / 1), the batch-1 cfg1 network on the small-map and the split-K routes and the forward
of two unfused training programs.  Batch 2 except where the route needs batch 1."""
import hashlib
import json
import os
import sys
import time

sys.path.insert(0, ".")
import torch

from sleap_nn_amd.architectures.model import PRECISIONS, Model

DEV = "cuda:0"
FUSION_OPTIONS = ("block_fuse", "mlp_fuse", "upsample_fold", "head_fuse", "dw_ln_fuse")  # (tests/test_gpu_plan_hazards.py)
OUT = None
N_CASES = 0


def unet_cfg(variant):
    bb = {"in_channels": 1, "kernel_size": 3, "filters": 16, "filters_rate": 2, "max_stride": 8, "stem_stride": None, "middle_block": True, "up_interpolate": True, "stacks": 1,
          "convs_per_block": 2, "output_stride": 2}
    bb.update({"bilinear": {}, "transposed": {"up_interpolate": False}, "cpb1": {"convs_per_block": 1, "middle_block": False, "filters_rate": 1}, "cpb3": {"convs_per_block": 3},
               "stem": {"stem_stride": 2, "max_stride": 4}, "k5": {"kernel_size": 5}, "filters24": {"filters": 24, "filters_rate": 1.5}}[variant])
    names = [f"n{i}" for i in range(5)]
    heads = {"confmaps": {"part_names": names, "output_stride": 2}, "pafs": {"edges": [[names[i], names[i + 1]] for i in range(4)], "output_stride": 4}}
    return bb, heads, "bottomup"


def convnext_cfg(channels):
    bb = {"model_type": None, "arch": {"depths": [2, 1, 1, 1], "channels": channels}, "in_channels": 1, "kernel_size": 3, "filters_rate": 2, "convs_per_block": 2, "up_interpolate": True,
          "stem_patch_kernel": 4, "stem_patch_stride": 2, "output_stride": 2, "max_stride": 32}
    return bb, {"confmaps": {"part_names": [str(i) for i in range(5)], "sigma": 2.5, "output_stride": 2}}, "single_instance"


def swin_cfg():
    bb = {"model_type": None, "arch": {"embed": 32, "depths": [2, 2, 2, 2], "num_heads": [1, 2, 4, 8]}, "in_channels": 1, "patch_size": 4, "window_size": 7, "kernel_size": 3,
          "filters_rate": 2, "convs_per_block": 2, "up_interpolate": True, "stem_patch_stride": 2, "output_stride": 2, "max_stride": 32, "pre_trained_weights": None}
    return bb, {"confmaps": {"part_names": [str(i) for i in range(5)], "sigma": 2.5, "output_stride": 2}}, "single_instance"


def convnextv2_cfg():
    hf = os.path.join("tests", "golden", "ckpt_dirs", "tiny_pretrained_convnextv2_single_instance", "hf_config")  # (settings only: depths 1 1 2 1, widths 16 32 48 64)
    bb = {"source": "hf", "model_name": hf, "in_channels": 3, "output_stride": 2, "max_stride": 32, "weights": False, "mode": "decoder", "out_indices": None, "freeze": False,
          "revision": None, "normalize": True, "image_mean": None, "image_std": None, "filters_rate": 1.5, "convs_per_block": 2, "kernel_size": 3, "up_interpolate": True}
    return bb, {"confmaps": {"part_names": ["a", "b", "c"], "sigma": 2.5, "output_stride": 2, "loss_weight": 1.0}}, "single_instance"


def make(backbone, bb, heads, mt, seed):
    """A model with seeded weights: Xavier matrices, and every vector (bias, affine, layer scale, GRN weight) moved off its neutral value so that each op shows in the output."""
    m = Model(backbone, bb, heads, mt).init_xavier_(seed=seed, head_scale=1.0)
    g = torch.Generator().manual_seed(seed + 1000)
    sd = m.state_dict()
    for k, shape in m.param_shapes.items():
        if len([n for n in shape if int(n) > 1]) <= 1:
            sd[k] = sd[k] + 0.05 * torch.randn(sd[k].shape, generator=g)
    m.load_state_dict(sd, strict=True)
    return m.to(DEV)


def image(batch, channels, hw, seed):
    return torch.randint(0, 256, (batch, channels, hw[0], hw[1]), dtype=torch.uint8, generator=torch.Generator().manual_seed(seed)).to(DEV)


def record(name, m, img):
    global N_CASES
    m(img)  # (sizes the workspace for this setting)
    torch.cuda.synchronize()
    m._workspace.zero_()
    out = m(img)
    torch.cuda.synchronize()
    row = {"case": name, "kernels": m.last_kernels(), "ranges": [[op, ln, int(is_dst), slot, off, n] for op, ln, is_dst, slot, off, n in m.last_ranges()],
           "sha256": {k: hashlib.sha256(out[k].cpu().contiguous().numpy().tobytes()).hexdigest() for k in sorted(out)}}
    OUT.write(json.dumps(row, sort_keys=True) + "\n")
    N_CASES += 1


def sweep(tag, backbone, bb, heads, mt, hw, precision, pins, channels=1):
    img = image(2, channels, hw, hw[1])
    m = make(backbone, bb, heads, mt, hw[0])
    m.set_precision(precision)
    for k, v in (pins or {}).items():
        m.set_option(k, v)
    for reuse in (1, 0):
        m.set_option("workspace_reuse", reuse)
        for off in (None,) + FUSION_OPTIONS:
            for k in FUSION_OPTIONS:
                m.set_option(k, 0 if k == off else 1)
            record(f"{tag} {precision} {hw[0]}x{hw[1]} reuse={reuse} {'pinned ' if pins else ''}{off or 'defaults'}{'=0' if off else ''}", m, img)
    for k in FUSION_OPTIONS:
        m.set_option(k, 1)
    if pins:
        for k in pins:
            m.set_option(k, 1)  # (the default of both routing options that get pinned)
        for reuse in (1, 0):
            m.set_option("workspace_reuse", reuse)
            record(f"{tag} {precision} {hw[0]}x{hw[1]} reuse={reuse} defaults", m, img)
    m.set_fusion(False)  # the op-by-op program on shared slots, as _sweep runs it
    m.set_option("conv_precision", PRECISIONS[precision])
    m.set_option("workspace_reuse", 1)
    m.set_option("pool_peephole", 1)
    m.set_option("fuse_gelu_fwd", 1)
    record(f"{tag} {precision} {hw[0]}x{hw[1]} unfused program, shared slots", m, img)


def main():
    global OUT
    t0 = time.time()
    OUT = open(sys.argv[1], "w")
    for variant in ("bilinear", "transposed", "cpb1", "cpb3", "stem", "k5", "filters24"):
        for hw in ((64, 96), (72, 104)):
            for precision in ("exact", "split", "fp16"):
                bb, heads, mt = unet_cfg(variant)
                fmt = "f32" if precision == "exact" or variant in ("stem", "k5") else precision
                plain = variant in ("bilinear", "transposed")
                pins = {"conv_f16_rows": 2} if (plain and fmt == "fp16") else ({"conv_smallmap": 2} if (plain and fmt == "f32") else None)
                sweep(f"unet {variant}", "unet", bb, heads, mt, hw, precision, pins)
    for channels in ([96, 192, 384, 768], [24, 40, 72, 136]):
        for precision in ("exact", "split", "fp16"):
            bb, heads, mt = convnext_cfg(channels)
            sweep(f"convnext {channels[0]}", "convnext", bb, heads, mt, (64, 96), precision, None)
    bb, heads, mt = convnext_cfg([96, 192, 384, 768])  # ConvNeXt on the fp16 pipe (convnext_f16): the fp16 depthwise / LayerNorm / row-GEMM routes
    m = make("convnext", bb, heads, mt, 5).set_precision("fp16", convnext_f16=True)
    for off in (None, "dw_ln_fuse"):
        m.set_option("dw_ln_fuse", 0 if off else 1)
        record(f"convnext 96 convnext_f16 {off or 'defaults'}", m, image(2, 1, (64, 96), 96))
    bb, heads, mt = swin_cfg()
    for swint_f16 in (False, True):
        m = make("swint", bb, heads, mt, 7).set_precision("fp16", swint_f16=swint_f16)
        record(f"swint small swint_f16={int(swint_f16)}", m, image(2, 1, (64, 96), 11))
    bb, heads, mt = convnextv2_cfg()
    m = make("pretrained", bb, heads, mt, 9)
    for reuse in (1, 0):
        m.set_option("workspace_reuse", reuse)
        for fuse in (0, 1):
            m.set_option("grn_fuse", fuse)
            record(f"convnextv2 A reuse={reuse} grn_fuse={fuse}", m, image(2, 3, (64, 96), 13))
    # batch 1, BASELINE cfg1's network: the small-map route (default), then K split over workgroups, then neither
    si_bb = {"in_channels": 1, "kernel_size": 3, "filters": 16, "filters_rate": 2, "max_stride": 16, "stem_stride": None, "middle_block": True, "up_interpolate": True, "stacks": 1,
             "convs_per_block": 2, "output_stride": 2}
    si_heads = {"confmaps": {"part_names": [f"k{i}" for i in range(5)], "sigma": 2.5, "output_stride": 2, "loss_weight": 1.0}}
    m = make("unet", si_bb, si_heads, "single_instance", 11)
    img = image(1, 1, (256, 256), 5)
    record("cfg1 batch 1 defaults", m, img)
    m.set_option("conv_smallmap", 0)
    record("cfg1 batch 1 conv_smallmap=0", m, img)
    m.set_option("conv_splitk", 0)
    record("cfg1 batch 1 conv_smallmap=0 conv_splitk=0", m, img)
    # the forward of an unfused training program (every activation kept): the pool peephole, Linear -> GELU / scale-add epilogues
    bb, heads, mt = unet_cfg("bilinear")
    m = make("unet", bb, heads, mt, 3).train(True)
    for peephole in (1, 0):
        m.set_option("pool_peephole", peephole)
        record(f"unet bilinear training program pool_peephole={peephole}", m, image(2, 1, (64, 96), 17))
    bb, heads, mt = convnext_cfg([24, 40, 72, 136])
    m = make("convnext", bb, heads, mt, 4).train(True)
    for fuse in (1, 0):
        m.set_option("fuse_gelu_fwd", fuse)
        record(f"convnext 24 training program fuse_gelu_fwd={fuse}", m, image(2, 1, (64, 96), 19))
    OUT.close()
    print(f"{N_CASES} cases in {time.time() - t0:.1f} s -> {sys.argv[1]}")


if __name__ == "__main__":
    main()
