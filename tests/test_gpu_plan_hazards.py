"""The workspace planner (build_plan) and the run-time router (ph_model_forward) must agree: when one launch also computes the op behind it, or writes the next op's
tensor one op early, no destination of that launch may lie on a byte range the launch -- or any later launch -- still reads.  The library reports what every launch of the
last forward was handed (``Model.last_ranges()``); ``_check_plan`` holds that record to the invariant itself, with liveness recomputed here from ``Model.ops`` and
``last_kernels()`` (not from the planner), over every program shape the project runs.  The numeric case at the end drives the persistent fp16 tile loops (stem_f16_kernel,
block2_c32_f16_kernel) through three and more rounds with an XCD boundary inside a frame, where a halo read of a recycled range would show up in the data.

Round 6's block_fuse broke the invariant on every plain-fp16 UNet plan: the fused launch read enc0's pooled tensor and wrote enc1's output through the same bytes
(``unet fp16 (64, 96) fused, defaults: launch of op 1 (kernel 14): destination slot 4 [0, 196608) lies on source slot 2 [0, 196608) of the same launch``, and the same at
72 x 104, with the transposed-conv decoder and at 3 x 512 x 1024); build_plan now holds the pair's releases for one op (csrc/plan.hip: fuses_block2, the router's own
predicate)."""
import pytest
import torch

from oracle import cpu_ref as O
from sleap_nn_amd import _lib as L
from tests.test_gpu_f16_pipe import FP16_ATOL

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# Kernels that may be handed a destination EXACTLY on one of their sources (same offset, same byte count).  Read the kernel before adding one; a partial overlap is never allowed.
IN_PLACE_OK = {
    L.KV_MLP: "cnblock_mlp_kernel: row-local -- a row tile loads all of its x rows before its first product and its residual elements in the epilogue right before the store of "
              "the same elements, no other tile reads those rows (lanes past the last row re-read row M - 1, but only into outputs that are never stored); "
              "ph_model_forward falls back to the two GEMMs for any other overlap",
}
FUSION_OPTIONS = ("block_fuse", "mlp_fuse", "upsample_fold", "head_fuse", "dw_ln_fuse")


def _hit(a, b):
    return a[0] < b[0] + b[1] and b[0] < a[0] + a[1]


def _check_plan(m, where):
    """The invariant on the last forward of ``m`` -> the set of run-time fusions that forward took (so that a case can assert it is not vacuous)."""
    ops, kv, rows = m.ops, m.last_kernels(), m.last_ranges()
    total = m._workspace.numel()
    launches, rng = {}, {}
    for op, ln, is_dst, slot, off, n in rows:
        assert 0 <= op < len(ops) and off >= 0 and n > 0 and off + n <= total, (where, op, slot, off, n, total)
        launches.setdefault((op, ln), ([], []))[1 if is_dst else 0].append((slot, off, n))
        assert rng.setdefault(slot, (off, n)) == (off, n), (where, "slot", slot, "was handed out at two ranges", rng[slot], (off, n))  # (slot -1: the scratch region, a range like any other)
    order = sorted(launches)
    has_rows = {op for op, _ in order}

    # ---- within one launch
    for (op, ln) in order:
        srcs, dsts = launches[(op, ln)]
        for i, (dslot, doff, dn) in enumerate(dsts):
            for sslot, soff, sn in srcs:
                if _hit((doff, dn), (soff, sn)):
                    exact = (doff, dn) == (soff, sn)
                    assert exact and kv[op] in IN_PLACE_OK, (f"{where}: launch of op {op} (kernel {kv[op]}): destination slot {dslot} [{doff}, {doff + dn}) lies on source slot {sslot} "
                                                             f"[{soff}, {soff + sn}) of the same launch")
            for eslot, eoff, en in dsts[i + 1:]:
                assert not _hit((doff, dn), (eoff, en)), f"{where}: launch of op {op}: destinations slot {dslot} [{doff}, {doff + dn}) and slot {eslot} [{eoff}, {eoff + en}) intersect"

    # ---- liveness from the program: which op's launch performs each read
    def_op = {}
    for p, o in enumerate(ops):
        for s in (o.dst, o.dst2):
            if s >= 0 and o.kind != L.OP_HEAD:
                assert s not in def_op, (where, "slot", s, "has two writers")
                def_op[s] = p

    def doer(p):  # op whose launch does op p's work
        if p in has_rows:
            return p
        o = ops[p]
        if o.kind == L.OP_UPSAMPLE:  # folded into the conv behind it, which reads the half-resolution tensor itself
            assert p + 1 in has_rows and ops[p + 1].kind == L.OP_CONV and ops[p + 1].src1 == o.dst, (where, p)
            return p + 1
        assert o.kind in (L.OP_CONV, L.OP_HEAD, L.OP_LINEAR, L.OP_POOL, L.OP_GELU, L.OP_SCALE_ADD, L.OP_LAYERNORM), (where, "op", p, "of kind", o.kind, "has no launch")
        if o.kind in (L.OP_CONV, L.OP_HEAD):
            assert kv[p] == L.KV_FUSED, (where, p, kv[p])
        if o.kind == L.OP_LINEAR:
            assert kv[p] == L.KV_MLP, (where, p, kv[p])
        q = doer(def_op[o.src0])  # absorbed by the producer of its input ...
        if o.kind != L.OP_HEAD:  # ... whose launch must then have been handed this op's dst (a head's output is not in the workspace), unless nobody reads it
            handed = {slot for key in order if key[0] == q for slot, _o, _n in launches[key][1]}
            assert {x for x in (o.dst, o.dst2) if x >= 0 and any(x in (r.src0, r.src1) for r in ops)} <= handed, (where, "op", p, "has no launch and op", q, "did not write its dst", sorted(handed))
        return q

    live_until = {}
    for p, o in enumerate(ops):
        for s in (o.src0, o.src1):
            if s >= 0:
                live_until[s] = max(live_until.get(s, -1), doer(p))
    written = {}
    for key in order:
        for slot, _off, _n in launches[key][1]:
            written.setdefault(slot, key)
        for slot, _off, _n in launches[key][0]:
            assert slot in written and written[slot] < key, (where, "launch", key, "reads slot", slot, "before any launch wrote it")
            live_until[slot] = max(live_until.get(slot, -1), key[0])
    for key in order:
        op = key[0]
        for dslot, doff, dn in launches[key][1]:
            for s, r in rng.items():
                if s == dslot or s not in written or not written[s] < key or live_until.get(s, -1) < op or not _hit((doff, dn), r):
                    continue
                in_place = r == (doff, dn) and kv[op] in IN_PLACE_OK and live_until[s] == op and any(x[0] == s for x in launches[key][0])
                assert in_place, (f"{where}: launch {key} (kernel {kv[op]}) writes slot {dslot} [{doff}, {doff + dn}) over slot {s} [{r[0]}, {r[0] + r[1]}), which op "
                                  f"{live_until[s]} still reads")

    seen = set()
    if L.KV_F16_BLOCK in kv:
        seen.add("block")
    if L.KV_STEM in kv:
        seen.add("stem")
    if L.KV_MLP in kv:
        seen.add("mlp")
    for p, o in enumerate(ops):
        if p in has_rows:
            continue
        doer(p)  # (holds the op to its kernel code and its dst to the launch that did its work)
        if o.kind == L.OP_UPSAMPLE:
            # folded only if the conv behind it READ the half-resolution tensor: no launch of that op was handed the up-sampled slot, one was handed the bilinear's source.
            # (A bilinear the router deferred and then produced inside the conv's op after all is a late launch, not a fold.)
            recs = [(is_dst, slot) for key in order if key[0] == p + 1 for is_dst in (0, 1) for slot, _o, _n in launches[key][is_dst]]
            seen.add("fold" if (0, o.src0) in recs and (1, o.dst) not in recs and (0, o.dst) not in recs else "late_upsample")
        else:
            seen.add({L.OP_CONV: "block", L.OP_LINEAR: "mlp", L.OP_HEAD: "head", L.OP_LAYERNORM: "dw_ln", L.OP_POOL: "pool_peephole", L.OP_GELU: "gelu_fwd", L.OP_SCALE_ADD: "gelu_fwd"}.get(o.kind, "other"))
    return seen


def _unet_cfg(variant):
    bb = {"in_channels": 1, "kernel_size": 3, "filters": 16, "filters_rate": 2, "max_stride": 8, "stem_stride": None, "middle_block": True, "up_interpolate": True, "stacks": 1,
          "convs_per_block": 2, "output_stride": 2}
    bb.update({"bilinear": {}, "transposed": {"up_interpolate": False}, "cpb1": {"convs_per_block": 1, "middle_block": False, "filters_rate": 1}, "cpb3": {"convs_per_block": 3},
               "stem": {"stem_stride": 2, "max_stride": 4},  # (a stem adds a pool of its own: the deepest map sits at stride 8 here too)
               "k5": {"kernel_size": 5}, "filters24": {"filters": 24, "filters_rate": 1.5}}[variant])
    names = [f"n{i}" for i in range(5)]
    heads = {"confmaps": {"part_names": names, "output_stride": 2}, "pafs": {"edges": [[names[i], names[i + 1]] for i in range(4)], "output_stride": 4}}
    return bb, heads, "bottomup"


def _convnext_cfg(channels):
    bb = {"model_type": None, "arch": {"depths": [2, 1, 1, 1], "channels": channels}, "in_channels": 1, "kernel_size": 3, "filters_rate": 2, "convs_per_block": 2, "up_interpolate": True,
          "stem_patch_kernel": 4, "stem_patch_stride": 2, "output_stride": 2, "max_stride": 32}
    return bb, {"confmaps": {"part_names": [str(i) for i in range(5)], "sigma": 2.5, "output_stride": 2}}, "single_instance"


def _sweep(backbone, bb, heads, mt, hw, precision, expect, pins=None):
    """One model through every fusion setting: defaults, each fusion option off in turn, the op-by-op program on shared slots.  ``expect(setting)`` -> (fusions that must
    have happened under that setting, fusions that cannot happen there); an option's own fusion must be gone when it is off.  ``pins``: routing options (not fusion options)
    held at a value in the fused program, where a fusion otherwise hangs on a run-time cost estimate."""
    from sleap_nn_amd.architectures.model import PRECISIONS, Model

    img = torch.randint(0, 256, (2, 1, hw[0], hw[1]), dtype=torch.uint8, generator=torch.Generator().manual_seed(hw[1])).to(DEV)
    m = Model(backbone, bb, heads, mt).init_xavier_(seed=hw[0], head_scale=1.0).to(DEV)
    m.set_precision(precision)
    for k, v in (pins or {}).items():
        m.set_option(k, v)
    gone = {"block_fuse": "block", "mlp_fuse": "mlp", "upsample_fold": "fold", "head_fuse": "head", "dw_ln_fuse": "dw_ln"}
    for off in (None,) + FUSION_OPTIONS:
        for k in FUSION_OPTIONS:
            m.set_option(k, 0 if k == off else 1)
        out = m(img)
        assert all(torch.isfinite(v).all() for v in out.values())
        assert m.get_option("workspace_reuse") == 1.0
        where = f"{backbone} {precision} {hw} fused, {off or 'defaults'}{' = 0' if off else ''}"
        seen = _check_plan(m, where)
        print(where, "->", sorted(seen))
        must, never = expect(off)
        assert "other" not in seen, (where, seen)
        assert must <= seen, (where, "expected fusions did not happen", sorted(must), sorted(seen))
        assert not (never & seen), (where, "fusions that cannot happen here", sorted(never & seen))
        if off:
            assert gone[off] not in seen, (where, seen)
    for k in FUSION_OPTIONS:
        m.set_option(k, 1)
    for k in (pins or {}):
        m.set_option(k, 1)  # (the default of both routing options that get pinned)
    m.set_fusion(False)  # the op-by-op program (conv -> pool, Linear -> GELU, Linear -> scale-add as separate ops): a C-API user can run it on shared slots
    m.set_option("conv_precision", PRECISIONS[precision])
    m.set_option("workspace_reuse", 1)
    m.set_option("pool_peephole", 1)
    m.set_option("fuse_gelu_fwd", 1)
    out = m(img)
    assert all(torch.isfinite(v).all() for v in out.values())
    where = f"{backbone} {precision} {hw} unfused program, shared slots"
    seen = _check_plan(m, where)
    print(where, "->", sorted(seen))
    must, never = expect("unfused")
    assert "other" not in seen and must <= seen and not (never & seen), (where, sorted(must), sorted(never), sorted(seen))


@pytest.mark.parametrize("precision", ["exact", "split", "fp16"])
@pytest.mark.parametrize("hw", [(64, 96), (72, 104)])  # (72 x 104: 9 x 13 pixels at the deepest level, odd pooled sizes)
@pytest.mark.parametrize("variant", ["bilinear", "transposed", "cpb1", "cpb3", "stem", "k5", "filters24"])
def test_unet_launches_never_write_what_is_still_read(variant, hw, precision):
    bb, heads, mt = _unet_cfg(variant)
    fmt = "f32" if precision == "exact" or variant in ("stem", "k5") else precision  # (7 x 7 / 5 x 5 convs keep the whole program in fp32: forward_format)
    plain = variant in ("bilinear", "transposed")  # 16 / 32 / 64 / 128 filters, two convs per block: the networks whose routing is reasoned out below
    # Whether a deferred bilinear is folded hangs on a cost estimate at the routing defaults (conv_f16_rows = 1: c_rows < 0.95 c_old; conv_smallmap = 1: sm_cost_us against the
    # other kernel).  With the routing pinned to "wherever the shape fits" it is decided by shapes: the decoder's first refine conv (64 + 128 -> 64 at stride 4: N tile 64, even
    # maps) is taken by conv3x3_f16_rows_kernel / conv3x3_sm_kernel, which read the half-resolution tensor themselves.
    pins = {"conv_f16_rows": 2} if (plain and fmt == "fp16") else ({"conv_smallmap": 2} if (plain and fmt == "f32") else None)

    def expect(setting):
        must, never = set(), {"mlp", "dw_ln", "gelu_fwd"}  # (no such op in a UNet program)
        if fmt != "f32":
            never.add("pool_peephole")  # the peephole lives in the fp32 conv path only
        if fmt == "split":
            never |= {"fold", "late_upsample", "head", "block"}  # split precision: no folded bilinear, no head in an epilogue, no two-conv block (all three ask for FMT_F16 / FMT_F32)
        if fmt == "f32":
            never.add("block")
        if variant == "transposed":
            never |= {"fold", "late_upsample"}  # no bilinear op in the program
        if setting == "unfused":
            never.add("stem")  # (the stem is a plan-level fusion of the fused program)
            if plain and fmt == "f32":
                must.add("pool_peephole")  # conv + ReLU -> pool pairs of 32 / 64 channels on the F(2x2,3x3) kernels: the epilogue writes the pool
            return must, never
        if plain:
            must.add("stem")  # two 3 x 3 convs of <= 16 filters + pool in front: the plan-level stem
        if fmt == "fp16" and variant in ("bilinear", "transposed", "cpb3") and setting != "block_fuse":
            must.add("block")  # conv(16 -> 32) + conv(32 -> 32) behind the first block: block2_c32_f16_kernel
        if variant == "bilinear" and fmt in ("f32", "fp16") and setting != "upsample_fold":
            must.add("fold")  # (pinned routing, see above)
        if plain and fmt in ("f32", "fp16") and setting != "head_fuse":
            # fp16: the PAF head reads the 64-channel conv at stride 4 (N tile 64): both fp16 conv kernels carry it in the epilogue.  fp32: the confidence-map head (5 <= 16
            # channels) reads the 32-channel conv at stride 2, which the pinned small-map kernel takes with every channel of a pixel in one workgroup.
            must.add("head")
        return must, never

    _sweep("unet", bb, heads, mt, hw, precision, expect, pins)


@pytest.mark.parametrize("precision", ["exact", "split", "fp16"])  # (ConvNeXt programs run exact fp32 whatever is asked for: all three must plan the same way)
@pytest.mark.parametrize("channels", [[96, 192, 384, 768], [24, 40, 72, 136]])
def test_convnext_launches_never_write_what_is_still_read(channels, precision):
    bb, heads, mt = _convnext_cfg(channels)

    def expect(setting):
        never = {"block", "stem", "pool_peephole"}  # (UNet-only fusions; ConvNeXt's pools sit behind Linear / LayerNorm ops)
        if setting == "unfused":
            return {"gelu_fwd"}, never | {"mlp"}  # Linear -> GELU and Linear -> scale-add written by the Linear's epilogue; the MLP kernel needs the fused ops
        must = set()
        if setting != "dw_ln_fuse":
            must.add("dw_ln")  # every CNBlock's LayerNorm rides in the depthwise kernel
        if channels[0] == 96:
            if setting != "mlp_fuse":
                must.add("mlp")  # 96- and 192-channel blocks: cnblock_mlp_kernel
        else:
            never.add("mlp")  # 24 / 40 / 72 / 136 channels: no width the kernel takes
        return must, never  # (a folded bilinear or a head in the decoder's epilogues hangs on cost estimates here: checked where it happens, not required)

    _sweep("convnext", bb, heads, mt, (64, 96), precision, expect)


def _bands(t, rows=8):
    """(B, C, H, W) -> (B, ceil(H / rows)): maximum of |t| over each band of ``rows`` output rows."""
    b, c, h, w = t.shape
    pad = (-h) % rows
    a = torch.nn.functional.pad(t.abs(), (0, 0, 0, pad))
    return a.reshape(b, c, (h + pad) // rows, rows, w).amax(dim=(1, 3, 4))


def test_three_rounds_of_the_persistent_fp16_tile_loops_are_batch_invariant_and_band_accurate():
    """Plain fp16, all defaults, frames of 512 x 1024: enc1 is a 256 x 512 map = 512 tiles of 8 x 32 per frame, and B is chosen so that block2_c32_f16_kernel's two workgroups
    per CU walk at least three tiles each while an XCD's contiguous tile range ends inside a frame (stem_f16_kernel, four workgroups per CU on the 512 x 1024 map, gets six
    rounds from the same forward).  (1) Every frame of the B-frame forward equals its own 1-frame forward bit for bit -- there the 512 tiles are one round, every halo is read a
    whole tile time before any store; (2) that 1-frame forward is within the fp16 bar of the fp32 oracle; (3) block_fuse on / off differ by a few fp16 roundings in EVERY band of
    eight output rows, measured against that band's own scale, so that a corrupted halo line cannot hide behind a global maximum."""
    from sleap_nn_amd.architectures.model import Model

    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    per_frame = (256 // 8) * (512 // 32)
    B = -(-3 * 2 * n_cu // per_frame)
    while ((B * per_frame + 7) // 8) % per_frame == 0:
        B += 1
    tiles = B * per_frame
    assert tiles >= 3 * 2 * n_cu and ((tiles + 7) // 8) % per_frame != 0, (B, tiles, n_cu)
    bb = {"in_channels": 1, "kernel_size": 3, "filters": 16, "filters_rate": 2, "max_stride": 8, "stem_stride": None, "middle_block": True, "up_interpolate": True, "stacks": 1,
          "convs_per_block": 2, "output_stride": 2}
    names = [f"n{i}" for i in range(5)]
    heads = {"confmaps": {"part_names": names, "output_stride": 2}, "pafs": {"edges": [[names[i], names[i + 1]] for i in range(4)], "output_stride": 4}}
    sd = O.init_state(bb, heads, "bottomup", seed=29, head_scale=1.0)
    img = torch.randint(0, 256, (B, 1, 512, 1024), dtype=torch.uint8, generator=torch.Generator().manual_seed(31))

    def run(x, block_fuse):
        m = Model("unet", bb, heads, "bottomup")
        m.load_state_dict(sd)
        m.to(DEV).set_precision("fp16")
        m.set_option("conv_f16_rows", 2)  # (1 chooses per layer by a cost estimate that depends on the batch: pinned, as is everything else last_kernels() shows)
        m.set_option("block_fuse", block_fuse)
        out = {k: v.cpu() for k, v in m(x.to(DEV)).items()}
        _check_plan(m, f"fp16 {tuple(x.shape)} block_fuse {block_fuse}")
        return out, m.last_kernels()

    full, kv = run(img, 1)
    assert L.KV_F16_BLOCK in kv and L.KV_STEM in kv, kv
    for b in range(B):
        one, kv1 = run(img[b:b + 1], 1)
        assert kv1 == kv, (b, kv1, kv)
        for k in full:
            same = torch.equal(full[k][b], one[k][0])
            if not same:
                bad = (full[k][b] != one[k][0]).nonzero()
                print(f"frame {b} head {k}: {bad.shape[0]} elements differ, rows {bad[:, 1].min().item()} .. {bad[:, 1].max().item()}, max |d| {(full[k][b] - one[k][0]).abs().max().item():.3e}")
            assert same, (b, k, "the frame in the batch is not the frame alone")
        if b == 0:
            ref = O.model_forward(sd, bb, heads, "bottomup", img[:1])
            for k, v in ref.items():
                err = (one[k] - v).abs().max().item()
                print(f"1-frame forward vs the fp32 oracle, {k}: {err:.3e}")
                assert err <= FP16_ATOL, (k, err)
    apart, kv0 = run(img, 0)
    assert L.KV_F16_BLOCK not in kv0, kv0
    for k in full:
        d, scale = _bands(full[k] - apart[k]), _bands(apart[k]).clamp(min=1.0)
        worst = (d / scale).max().item()
        print(f"block_fuse 1 vs 0, {k}: worst band {worst:.3e} of its scale (bar 3e-3), global max |d| {d.max().item():.3e}")
        assert (d <= 3e-3 * scale).all(), (k, worst, (d > 3e-3 * scale).nonzero()[:8].tolist())
