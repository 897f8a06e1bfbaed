"""Record of the weight forms a handle owns: the check of a change to the host code that packs, derives and refreshes them (csrc/weights.hip, and the call into it from
ph_model_set_params in csrc/train.hip) that must not move a byte.  The sibling of tools/forward_trace.py and tools/backward_trace.py, whose config builders, ``make`` and
``record`` helpers it reuses.

    python tools/weights_trace.py OUT.jsonl

Ten models (UNet bilinear, transposed, cpb3, stem, k5, filters24; ConvNeXt 96 and 24; Swin; ConvNeXtV2) on frames of 64 x 96, batch 2.  Per model one JSON line per step:

a. handle created from weights A, one forward each at exact, split and fp16 precision (``convnext_f16`` / ``swint_f16`` on the fp16 one, so that the lazy fp16 packs
   exist): n0 = the number of allocations, and ``[bytes, sha256]`` of each (``ph_model_debug_allocs``);
b. ``ph_model_set_params`` with the arena of weights B on that handle, set to ``workspace_reuse`` 0 and exact precision: the same list over the allocations below n0
   (the gather and pack tables allocated behind them hold device pointers and are not hashed) -- the forms that call leaves stale still hold A;
c. one further forward with ``workspace_reuse`` 1 (the Linear programs at fp16 on their fp16 pipe): the same list -- which forward refreshes the stale forms.

d. On the bilinear and the transposed UNet, ``workspace_reuse`` 1: kernels, ranges and output hashes (the rows of ``forward_trace.record``) with each option on its own
   that routes a layer to a form no default plan reads, and one training step each with ``conv_c16`` 0 and ``dgrad_wino`` 0 (the rows of ``backward_trace.record``).

Run it on a build of the commit before the change and on a build of the change, on the same device: the packers are host code, the pack kernels deterministic, so the two
files are byte-identical unless a form, its size, its place in the allocation order or the moment it is refreshed changed.  The wall time of create + first forward per model
goes to stdout only (the host cost of ph_model_create)."""
import ctypes as C
import hashlib
import json
import sys
import time

sys.path.insert(0, ".")
import torch

import tools.backward_trace as BT
import tools.forward_trace as FT
from sleap_nn_amd import _lib as L
from sleap_nn_amd.training.module import TrainingModule
from tools.forward_trace import DEV, convnext_cfg, convnextv2_cfg, image, make, swin_cfg, unet_cfg

HW = (64, 96)
ROUTE_OPTIONS = (("conv_wino", 0, 1), ("conv_wino", 2, 1), ("conv_wino2d", 0, 1), ("conv_w16", 0, 1), ("conv_wino4", 0, 1), ("conv_wino4", 3, 1), ("conv_n32_wino2d", 0, 1),
                 ("conv_dma", 0, 1), ("conv_dma32", 0, 1), ("conv_c16", 0, 1), ("stem_wino", 0, 2), ("stem_wino", 1, 2), ("conv_smallmap", 2, 1), ("conv_gemm_fill", 10, 0.8),
                 ("convt_phase", 0, 1), ("convt_one_launch", 0, 1))  # (name, value, default)


def models():
    """(tag, backbone, config triple, input channels, fp16 keyword of set_precision or None)."""
    for variant in ("bilinear", "transposed", "cpb3", "stem", "k5", "filters24"):
        yield f"unet {variant}", "unet", unet_cfg(variant), 1, None
    yield "convnext 96", "convnext", convnext_cfg([96, 192, 384, 768]), 1, "convnext_f16"
    yield "convnext 24", "convnext", convnext_cfg([24, 40, 72, 136]), 1, "convnext_f16"
    yield "swint small", "swint", swin_cfg(), 1, "swint_f16"
    yield "convnextv2 tiny", "pretrained", convnextv2_cfg(), 3, "convnext_f16"


def fp16_kwargs(f16_option):
    return {f16_option: True} if f16_option else {}


def alloc_rows(m, n0):
    return [[int(t.numel()), hashlib.sha256(t.numpy().tobytes()).hexdigest()] for t in m.debug_allocs(read_first=n0)]


def set_params(m, flat_dev):
    L.check(L.lib().ph_model_set_params(m._handle, C.c_void_p(flat_dev.data_ptr()), L.current_stream_ptr()))
    torch.cuda.synchronize()


def weight_steps(out, tag, backbone, cfg, channels, f16_option):
    img = image(2, channels, HW, 7)
    m = make(backbone, *cfg, 21)
    t0 = time.perf_counter()
    m(img)
    torch.cuda.synchronize()
    print(f"create + first forward: {tag}: {(time.perf_counter() - t0) * 1e3:.1f} ms", flush=True)
    m.set_precision("split")(img)
    m.set_precision("fp16", **fp16_kwargs(f16_option))(img)
    n0 = len(m.debug_allocs())
    out.write(json.dumps({"model": tag, "step": "a", "n0": n0, "allocs": alloc_rows(m, n0)}, sort_keys=True) + "\n")
    flat_b = make(backbone, *cfg, 22).flat_params().to(DEV)
    m.set_precision("exact").set_option("workspace_reuse", 0)
    set_params(m, flat_b)
    out.write(json.dumps({"model": tag, "step": "b", "n_allocs": len(m.debug_allocs()), "allocs": alloc_rows(m, n0)}, sort_keys=True) + "\n")
    m.set_option("workspace_reuse", 1)
    if f16_option:
        m.set_precision("fp16", **fp16_kwargs(f16_option))
    m(img)
    out.write(json.dumps({"model": tag, "step": "c", "n_allocs": len(m.debug_allocs()), "allocs": alloc_rows(m, n0)}, sort_keys=True) + "\n")


def route_steps(variant):
    bb, heads, mt = unet_cfg(variant)
    img = image(2, 1, HW, 7)
    m = make("unet", bb, heads, mt, 21)
    m.set_option("workspace_reuse", 1)
    for key, value, default in ROUTE_OPTIONS:
        m.set_option(key, value)
        FT.record(f"weights d: unet {variant} {key}={value}", m, img)
        m.set_option(key, default)
    for key in ("conv_c16", "dgrad_wino"):
        tm = TrainingModule(make("unet", bb, heads, mt, 21), DEV)
        tm.model.set_option(key, 0)
        BT.record(f"weights d: unet {variant} training step {key}=0", tm, img, BT.targets_for(tm, img, 23))


def main():
    t0 = time.time()
    out = open(sys.argv[1], "w")
    FT.OUT = BT.OUT = out
    with torch.cuda.device(torch.device(DEV)):
        make("unet", *unet_cfg("cpb1"), 1)(image(2, 1, HW, 7))  # (the library load and the runtime's first launches stay out of the first model's time)
        torch.cuda.synchronize()
        for tag, backbone, cfg, channels, f16_option in models():
            weight_steps(out, tag, backbone, cfg, channels, f16_option)
        for variant in ("bilinear", "transposed"):
            route_steps(variant)
    out.close()
    print(f"{FT.N_CASES + BT.N_CASES} route cases, 30 weight steps in {time.time() - t0:.1f} s -> {sys.argv[1]}")


if __name__ == "__main__":
    main()
