"""conv3x3_wino4_kernel's raw halo slot is channel-planar ([channel][halo row][column]): the loader scatters a pixel's four channels over the planes,
the input transform reads a patch row as one 16-byte + one 8-byte access (low resolution: two 8-byte accesses).  A wrong piece-to-pixel map, plane
offset or row pitch shows as wrong halo columns / rows of single tiles, so the shapes here put tile edges, image borders, slot reuse and padded
channel quarters where such an error would sit.  Small networks through ``Model`` with ``conv_wino4 = 3`` (the kernel wherever the shape fits)."""
import pytest
import torch

from oracle import cpu_ref as O
from tests.test_gpu_parity import W4_RTOL  # the F(4x4,3x3) layers' bar against the oracle, of the head's scale: stated once, there

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
KERNELS_RTOL = 3e-5  # against the same network without the F(4x4,3x3) kernel, of the head's scale (as test_half_empty_n_tiles_and_rotated_tile_dealing_match_oracle states it inline)

CASES = {
    # 36 x 52 at the kernel's level: 3 x 2 workgroup tiles, the last row of tiles 4 rows high, the last column 20 wide (the second loader piece, the row and column
    # remainders); the decoder conv reads 64 + 128 channels, the 128 from the 18 x 26 map through the folded bilinear with every image border in a clamped halo
    "cut_tiles_36x52": dict(filters=64, rate=2, max_stride=2, hw=(36, 52), batch=2, ref_frames=2, min_wino4=3, fold=True),
    # two decoder levels with the folded bilinear: 20 x 36 from a 10 x 18 map (= one low-resolution halo: clamped on all four sides of one tile, the odd
    # low-resolution origin of tiles 1..7) and 40 x 72 from 20 x 36
    "fold_all_borders": dict(filters=64, rate=2, max_stride=4, hw=(40, 72), batch=3, ref_frames=3, min_wino4=6, fold=True),
    # 6 frames of 192 x 128 at 64 channels: 288 (pixel tile, N tile) units > 256 workgroups: a workgroup's second tile starts in the slots its first one left
    "more_units_than_workgroups": dict(filters=64, rate=2, max_stride=2, hw=(192, 128), batch=6, ref_frames=6, min_wino4=3, fold=True),
    # 72 / 108 / 162 channels: every source of every layer ends in padded quarters (72 -> 80, 108 -> 112, 162 -> 176), on both sources of the two decoder convs;
    # the last N tile of every layer is half empty or less
    "padded_quarters": dict(filters=72, rate=1.5, max_stride=4, hw=(48, 64), batch=2, ref_frames=2, min_wino4=7, fold=True),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_channel_planar_raw_slot_matches_oracle_and_the_other_kernels(case):
    from sleap_nn_amd import _lib as L
    from sleap_nn_amd.architectures.model import Model

    c = CASES[case]
    bb = {"in_channels": 1, "kernel_size": 3, "filters": c["filters"], "filters_rate": c["rate"], "max_stride": c["max_stride"], "stem_stride": None,
          "middle_block": True, "up_interpolate": True, "stacks": 1, "convs_per_block": 2, "output_stride": 1}
    heads = {"confmaps": {"part_names": ["a", "b", "c"], "output_stride": 1}}
    sd = O.init_state(bb, heads, "single_instance", seed=c["hw"][0] + c["filters"], head_scale=1.0)
    g = torch.Generator().manual_seed(c["hw"][1])
    img = torch.randint(0, 256, (c["batch"], 1) + c["hw"], dtype=torch.uint8, generator=g)
    ref = O.model_forward(sd, bb, heads, "single_instance", img[:c["ref_frames"]])["SingleInstanceConfmapsHead"]
    outs = {}
    for name, w4 in (("wino4", 3), ("other", 0)):
        m = Model("unet", bb, heads, "single_instance")
        m.load_state_dict(sd)
        m.set_option("conv_wino4", w4).set_option("conv_smallmap", 0)
        m.to(DEV)
        outs[name] = m(img.to(DEV))["SingleInstanceConfmapsHead"].cpu()
        kv = m.last_kernels()
        n4 = sum(1 for k in kv if k == L.KV_WINO4)
        if name == "wino4":
            assert n4 >= c["min_wino4"], (n4, [L.KV_NAMES.get(k, k) for k in kv])
            if c["fold"]:
                ups = [i for i, op in enumerate(m.ops) if op.kind == L.OP_UPSAMPLE]
                assert ups and all(kv[i + 1] == L.KV_WINO4 for i in ups), "every decoder's bilinear x2 must ride in the F(4x4,3x3) kernel"
            assert torch.equal(m(img.to(DEV))["SingleInstanceConfmapsHead"].cpu(), outs["wino4"])  # run-to-run bitwise
        else:
            assert n4 == 0
    scale = ref.abs().max().item()
    err_ref = (outs["wino4"][:c["ref_frames"]] - ref).abs().max().item()
    err_other = (outs["wino4"] - outs["other"]).abs().max().item()
    print(f"{case}: scale {scale:.4g}, vs oracle {err_ref / scale:.3g} of scale, vs the other kernels {err_other / outs['other'].abs().max().item():.3g}")
    assert err_ref <= W4_RTOL * scale, (err_ref, scale)
    assert err_other <= KERNELS_RTOL * outs["other"].abs().max().item(), (err_other, scale)
