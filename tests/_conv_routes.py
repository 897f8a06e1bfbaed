"""The case table of the exact-fp32 3x3 conv route (``ph_debug_conv3x3_route``; tests/test_conv_routes_cpu.py, tests/golden/conv3x3_routes.json).

Pure data: ``cases()`` returns the same list of ``ph_conv_route_case`` field dicts every time.  The golden file holds, case by case, what the routing
predicates answered BEFORE they were folded into ``conv3x3_route`` (recorded once on an MI355X, whose CU count is in the file), so the table may only
grow together with a new record.

The table varies one thing at a time around the arguments of an inference plan under default options: every (map, channel set) pair, then each argument
flag, each missing weight form and each option value on its own, then the arguments of a training plan's forward and of the data gradient.
"""
from __future__ import annotations

FIELDS = ("c0p", "c1p", "coutp", "bn", "B", "H", "W", "forms", "flags", "head_cout", "head_wcp", "use_dma", "dma32", "use_wino", "persist", "use_c16", "use_w16",
          "use_wino2d", "use_wino4", "wino4_min_cin", "use_sm", "splitk", "ptr_salt")  # int32 each, then int64 split_scratch_bytes

# weight forms that exist (bit mask `forms`)
F_DMA, F_WINO, F_WINO2, F_W16, F_C16, F_WINO4, F_SM = 1, 2, 4, 8, 16, 32, 64
# argument flags (bit mask `flags`)
A_SRC1, A_LOWRES, A_POOL, A_SKIP_DST, A_ACCUMULATE, A_RELU_MASK, A_HEAD = 1, 2, 4, 8, 16, 32, 64
# ConvKernel (csrc/conv3x3_route.h)
K_REGSTAGED, K_DMA9, K_WINO1D, K_C16, K_W16, K_WINO2D, K_WINO4, K_SMALLMAP = range(8)
KERNEL_NAMES = ("register-staged", "9-tap LDS-DMA", "F(2,3)", "conv3x3_c16", "wave-private F(2x2,3x3)", "wave-split F(2x2,3x3)", "F(4x4,3x3)", "small-map")
# property bits of the route
P_MASK, P_POOLS, P_HEAD_W2D, P_HEAD_W16, P_LOWRES, P_HEAD_SM = 1, 2, 4, 8, 16, 32

# (B, H, W): the fp32 3x3 layers' maps of the bench configurations at their bench batch, then the edge maps
MAPS = (
    [(1, s, s) for s in (256, 128, 64, 32, 16)]            # cfg1: single-instance UNet, 256 x 256, one frame
    + [(8, s, s) for s in (512, 128, 32)]                  # cfg2: 512 x 512, eight frames
    + [(32, s, s) for s in (512, 256, 128, 64, 32)]        # cfg3: 1024 x 1024, 32 frames
    + [(64, s, s) for s in (192, 48, 24)]                  # cfg4: 384 x 384 crops, 64 of them (the decoder's maps)
    + [(16, s, s) for s in (384, 96)]                      # cfg5: 768 x 768, 16 frames
    + [(4, 160, 280), (4, 80, 140), (4, 40, 70), (4, 20, 35)]  # the published workload
    + [(1, 8, 8), (2, 16, 16), (4, 72, 104), (4, 62, 90), (2, 30, 42), (1, 31, 45)]  # edges: tiny, no multiple of 16, no multiple of 4, even / odd with a half-resolution src1
)

# (c0p, c1p, coutp, N tile)
CHANNELS = ((16, 0, 16, 32), (16, 0, 32, 32), (32, 0, 32, 32), (16, 32, 16, 32), (32, 64, 32, 32), (32, 64, 32, 64), (64, 0, 64, 64), (64, 128, 64, 64),
            (256, 512, 256, 64), (64, 0, 96, 64))

SCRATCH_BIG, SCRATCH_SMALL = 1 << 40, 4096

DEFAULT_OPTIONS = dict(use_dma=1, dma32=1, use_wino=1, persist=1, use_c16=1, use_w16=1, use_wino2d=1, use_wino4=1, wino4_min_cin=64, use_sm=1, splitk=1)
OPTION_VALUES = (("use_dma", (0,)), ("dma32", (0,)), ("use_wino", (0, 2)), ("persist", (0,)), ("use_c16", (0,)), ("use_w16", (0,)), ("use_wino2d", (0,)),
                 ("use_wino4", (0, 2)), ("wino4_min_cin", (16, 128)), ("use_sm", (0, 2)), ("splitk", (0, 2, 4)))


def w16_shape_ok(c0p: int, c1p: int, coutp: int) -> bool:
    if coutp not in (16, 32):
        return False
    if c1p == 0:
        return c0p in (16, 32)
    return 2 <= (c0p + c1p) // 16 <= (4 if coutp == 16 else 2)


def default_forms(c0p: int, c1p: int, coutp: int, bn: int) -> int:
    """The forms ph_model_create derives for such a layer (csrc/weights.hip: forms_conv3x3_forward)."""
    f = F_DMA | F_WINO | F_SM
    if bn == 64:
        f |= F_WINO2
        if c0p + c1p >= 64:
            f |= F_WINO4
    if bn == 32 and w16_shape_ok(c0p, c1p, coutp):
        f |= F_W16
    if (c0p, c1p, coutp) == (16, 0, 16):
        f |= F_C16
    return f


def _case(m, ch, **over):
    c0p, c1p, coutp, bn = ch
    c = dict(c0p=c0p, c1p=c1p, coutp=coutp, bn=bn, B=m[0], H=m[1], W=m[2], forms=default_forms(*ch), flags=A_SRC1 if c1p else 0, head_cout=0, head_wcp=0,
             ptr_salt=0, split_scratch_bytes=SCRATCH_BIG, **DEFAULT_OPTIONS)
    c.update(over)
    return c


def cases():
    out = []
    for m in MAPS:
        for ch in CHANNELS:
            c0p, c1p, coutp, bn = ch
            base = _case(m, ch)
            out.append(base)
            src1 = base["flags"]
            # ---- argument flags, each on its own (and the pairs that occur together)
            flag_sets = [A_POOL, A_POOL | A_SKIP_DST, A_HEAD]
            if c1p:
                flag_sets += [A_LOWRES, A_LOWRES | A_HEAD]
            for fl in flag_sets:
                out.append(_case(m, ch, flags=src1 | fl, head_cout=5 if fl & A_HEAD else 0, head_wcp=coutp if fl & A_HEAD else 0))
            out.append(_case(m, ch, split_scratch_bytes=0))
            out.append(_case(m, ch, split_scratch_bytes=SCRATCH_SMALL))
            # ---- each weight form missing in turn
            for bit in (F_DMA, F_WINO, F_WINO2, F_W16, F_C16, F_WINO4, F_SM):
                if base["forms"] & bit:
                    out.append(_case(m, ch, forms=base["forms"] & ~bit))
                    if c1p:
                        out.append(_case(m, ch, forms=base["forms"] & ~bit, flags=src1 | A_LOWRES))
            # ---- each option at each of its other documented values
            for name, values in OPTION_VALUES:
                for v in values:
                    out.append(_case(m, ch, **{name: v}))
                    if name in ("use_sm", "use_wino4", "splitk") and c1p:
                        out.append(_case(m, ch, flags=src1 | A_LOWRES, **{name: v}))
            out.append(_case(m, ch, splitk=2, split_scratch_bytes=SCRATCH_SMALL))
            out.append(_case(m, ch, use_sm=0, split_scratch_bytes=SCRATCH_SMALL))
            out.append(_case(m, ch, use_sm=0, use_wino4=0))
            out.append(_case(m, ch, use_sm=0, use_wino4=0, split_scratch_bytes=SCRATCH_SMALL))
            # ---- the forward of a training plan: no automatic split, no small-map kernel, F(4x4,3x3) on request only; the pool peephole's question
            train = dict(use_wino4=0, use_sm=0, splitk=0, split_scratch_bytes=0)
            for fl in (0, A_POOL, A_HEAD):
                out.append(_case(m, ch, flags=src1 | fl, head_cout=5 if fl & A_HEAD else 0, head_wcp=coutp if fl & A_HEAD else 0, **train))
            out.append(_case(m, ch, **dict(train, use_wino4=1)))
            out.append(_case(m, ch, **dict(train, use_sm=2), flags=src1 | A_POOL))
            # ---- the data gradient: one source, no scratch, accumulate / ReLU mask, dgrad_wino = 0 (use_wino = 0), F(4x4,3x3) on request
            if not c1p:
                dgrad = dict(use_wino4=0, use_sm=0, splitk=1, split_scratch_bytes=0)
                for fl in (0, A_ACCUMULATE, A_RELU_MASK, A_ACCUMULATE | A_RELU_MASK):
                    for uw in (1, 0):
                        out.append(_case(m, ch, flags=fl, use_wino=uw, **dgrad))
                    out.append(_case(m, ch, flags=fl, **dict(dgrad, use_wino4=1)))
                    out.append(_case(m, ch, flags=fl, **dict(dgrad, use_dma=0)))
                out.append(_case(m, ch, flags=A_RELU_MASK, **dict(dgrad, dma32=0)))
                out.append(_case(m, ch, flags=A_RELU_MASK, **dict(dgrad, use_w16=0)))
    return out
