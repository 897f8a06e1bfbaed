"""GPU parity tests: the HIP path (through the C ABI) vs the oracle and the golden fixtures.

Tolerances: confidence maps / PAFs within 1e-4 absolute of the reference (north_star);
peak indices, channels, sample ids, values and grouping membership bit-exact; refined
coordinates within 1e-5 px (25-term fp32 sums, different summation order than ATen).
"""
import json

import numpy as np
import pytest
import torch

from oracle import cpu_ref as O
from tests import _golden as G

pytestmark = pytest.mark.gpu

CMS_ATOL = 1e-4
# Heads of the synthetic-weight networks are scaled x0.05 (outputs O(1e-3)), where a bare 1e-4 absolute bar proves little: those
# tests also hold the error to this fraction of the head's max magnitude (measured: 1-2e-6 with the F(2x2,3x3) kernels).
HEAD_RTOL = 1e-5


def _head_close(got, ref, key=None):
    err = (got.cpu() - ref).abs().max().item()
    scale = ref.abs().max().item()
    assert err <= CMS_ATOL, (key, err, scale)
    assert err <= HEAD_RTOL * scale, (key, err, scale)
DEV = "cuda:0"

# convs_per_block 3 (bilinear / transposed-conv at rate 1.5) and 1: the reference's decoder keeps two refine convs per block (unet.py:203-216)
CPB_GOLDENS = ["unet_tiny_cpb3.npz", "unet_tiny_cpb3_trans.npz", "unet_tiny_cpb1.npz"]


def _assert_block_structure_activations_found(name, cfg, found):
    """The tensors whose existence is the point of the convs_per_block goldens must have been read back and compared, not skipped."""
    if name not in CPB_GOLDENS:
        return
    assert any(k.endswith("_refine_conv1") for k in found), (name, found)
    if cfg["backbone"]["convs_per_block"] == 3:
        assert any("encoder_stack" in k and k.endswith("_conv2") for k in found), (name, found)
        assert any(k.endswith("_middle_expand_conv1") for k in found), (name, found)


def _model(cfg, weights):
    from sleap_nn_amd.architectures.model import Model

    m = Model("unet", cfg["backbone"], cfg["heads"], cfg["model_type"])
    m.load_state_dict(weights, strict=True)
    return m.to(DEV)


@pytest.mark.parametrize("name", ["unet_tiny_interp.npz", "unet_tiny_trans.npz", "unet_tiny_bu13.npz", "unet_tiny_rgb.npz", "ckpt_bottomup.npz", "ckpt_single_instance.npz",
                                  "unet_tiny_stem.npz", "unet_tiny_k5.npz", "unet_f16_wino.npz"] + CPB_GOLDENS)
def test_forward_matches_reference_golden(name):
    z = G.load(name)
    cfg = G.config(z)
    m = _model(cfg, G.weights(z)).set_keep_activations(True)  # intermediate activations are read back below
    img = torch.from_numpy(z["image"]).squeeze(1).to(DEV)
    out = m(img)
    torch.cuda.synchronize()
    for k in [f for f in z.files if f.startswith("out/")]:
        ref = torch.from_numpy(z[k])
        got = out[k[4:]].cpu()
        assert got.shape == ref.shape
        err = (got - ref).abs().max().item()
        assert err <= CMS_ATOL, (k, err)
    n_act = 0
    found = []
    for k in [f for f in z.files if f.startswith("act/")]:
        ref = torch.from_numpy(z[k])
        try:
            got = m.read_activation(k[4:], ref.shape[0], ref.shape[-2:]).cpu()
        except KeyError:
            continue  # fused away by the stem kernel: never materialised in HBM
        err = (got - ref).abs().max().item()
        assert err <= CMS_ATOL, (k, err)
        n_act += 1
        found.append(k[4:])
    assert n_act >= 2 or not any(f.startswith("act/") for f in z.files)
    _assert_block_structure_activations_found(name, cfg, found)
    if name in CPB_GOLDENS:
        from sleap_nn_amd import _lib as L

        assert m.ops[0].kind != L.OP_STEM and L.KV_STEM not in m.last_kernels()  # neither block shape is the two-conv stem


@pytest.mark.parametrize("name", ["unet_tiny_interp.npz", "unet_tiny_rgb.npz", "ckpt_bottomup.npz"] + CPB_GOLDENS)
def test_unfused_program_matches_too(name):
    """The plan-level stem fusion is optional: the op-by-op program must give the same maps."""
    z = G.load(name)
    cfg = G.config(z)
    m = _model(cfg, G.weights(z)).set_fusion(False)
    img = torch.from_numpy(z["image"]).squeeze(1).to(DEV)
    out = m(img)
    for k in [f for f in z.files if f.startswith("out/")]:
        assert (out[k[4:]].cpu() - torch.from_numpy(z[k])).abs().max().item() <= CMS_ATOL
    for k in [f for f in z.files if f.startswith("act/")]:
        ref = torch.from_numpy(z[k])
        got = m.read_activation(k[4:], ref.shape[0], ref.shape[-2:]).cpu()
        assert (got - ref).abs().max().item() <= CMS_ATOL, k
    _assert_block_structure_activations_found(name, cfg, [k[4:] for k in z.files if k.startswith("act/")])  # (every one was read above)


def test_stem_fusion_odd_sizes_vs_unfused():
    """Odd H/W exercise the zero-padded pooling and partial tiles of the fused stem (compared with
    the unfused kernels, which the golden tests pin)."""
    from sleap_nn_amd.architectures.model import Model

    bb = {"in_channels": 1, "kernel_size": 3, "filters": 12, "filters_rate": 2, "max_stride": 2, "stem_stride": None, "middle_block": True, "up_interpolate": True, "stacks": 1, "convs_per_block": 2, "output_stride": 2}
    heads = {"confmaps": {"part_names": ["a", "b", "c"], "output_stride": 2}}
    sd = O.init_state(bb, heads, "single_instance", seed=3, head_scale=1.0)
    for hw in ((37, 45), (8, 32), (9, 33), (64, 70)):
        g = torch.Generator().manual_seed(hw[0])
        img = torch.randint(0, 256, (2, 1, hw[0], hw[1]), dtype=torch.uint8, generator=g)
        ref = O.model_forward(sd, bb, heads, "single_instance", img)["SingleInstanceConfmapsHead"]
        for stem_wino in (2, 1, 0):  # second conv as Winograd F(2x2,3x3) (the default), F(2,3) along x, direct
            m = Model("unet", bb, heads, "single_instance")
            m.load_state_dict(sd)
            m.set_option("stem_wino", stem_wino)
            assert m.ops[0].kind == 7  # fused stem in the plan
            # output_stride 2 with max_stride 2: the head sits on the middle block (no decoder) -> only the pooled path
            out = m.to(DEV)(img.to(DEV))["SingleInstanceConfmapsHead"].cpu()
            assert out.shape == ref.shape
            assert (out - ref).abs().max().item() <= CMS_ATOL, (hw, stem_wino)


def test_forward_float_inputs_and_odd_batch():
    z = G.load("unet_tiny_interp.npz")
    cfg = G.config(z)
    sd = G.weights(z)
    m = _model(cfg, sd)
    g = torch.Generator().manual_seed(5)
    img = torch.randint(0, 256, (3, 1, 40, 56), dtype=torch.uint8, generator=g)
    ref = O.model_forward(sd, cfg["backbone"], cfg["heads"], cfg["model_type"], img)
    from sleap_nn_amd.inference.backends import HipBackend

    be = HipBackend(m, DEV)
    for x in (img.unsqueeze(1), img.float(), img.float() / 255):  # uint8 5-D, float 0..255, float 0..1
        out = be(x)
        for k, v in ref.items():
            assert (out[k].cpu() - v).abs().max().item() <= CMS_ATOL


def test_forward_rejects_unaligned_sizes():
    from sleap_nn_amd._lib import PosehipError

    z = G.load("unet_tiny_interp.npz")
    m = _model(G.config(z), G.weights(z))
    with pytest.raises(PosehipError):
        m(torch.zeros((1, 1, 36, 44), dtype=torch.uint8, device=DEV))  # 36/8 not integral -> concat mismatch


def _refine_tol(cms, pts_int, map_inds, patch=5):
    """Per-peak tolerance for integral refinement: the offsets are ratios of 25-term fp32 sums whose
    summation order differs from ATen's (which itself depends on the host's SIMD width), so the
    admissible error grows with the conditioning sum|v| / |sum v| of the patch (maps with negative
    values can make it large; for real confidence maps it is ~1)."""
    flat = cms.reshape(-1, cms.shape[-2], cms.shape[-1]).cpu()
    pad = torch.nn.functional.pad(flat, (patch, patch, patch, patch))
    tol = []
    h = patch // 2
    for (x, y), mi in zip(pts_int.tolist(), map_inds.tolist()):
        crop = pad[int(mi), int(y) + patch - h : int(y) + patch + h + 1, int(x) + patch - h : int(x) + patch + h + 1]
        cond = float(crop.abs().sum() / crop.sum().abs().clamp_min(1e-30))
        tol.append(1e-5 + 4e-6 * cond)
    return np.asarray(tol)[:, None]


def test_local_and_global_peaks_match_reference():
    from sleap_nn_amd.inference.ops import peaks as HP

    z = G.load("peaks.npz")
    cases = sorted({k.split("/")[0] for k in z.files if "/" in k})
    n_checked = 0
    for c in cases:
        cms = torch.from_numpy(z[f"{c}/cms"]).to(DEV)
        for key in sorted({k.rsplit("/", 1)[0] for k in z.files if k.startswith(c + "/local_") or k.startswith(c + "/global_")}):
            parts = key.split("/")[1].split("_")
            if parts[0] == "local":
                if parts[2].startswith("p"):
                    ps = int(parts[2][1:])
                    pts, _, sb, sc = HP.find_local_peaks(cms, 0.2, "integral", ps)
                    rough = z[f"{c}/local_none_0.2/pts"]
                    tol = _refine_tol(cms, torch.from_numpy(rough), sb.cpu().long() * cms.shape[1] + sc.cpu().long(), ps)
                    assert (np.abs(pts.cpu().numpy() - z[key + "/pts"]) <= tol + 1e-4 * np.abs(z[key + "/pts"])).all(), key
                    continue
                ref = None if parts[1] == "none" else "integral"
                pts, vals, sb, sc = HP.find_local_peaks(cms, float(parts[2]), ref, 5)
                assert np.array_equal(sb.cpu().numpy(), z[key + "/sb"]), key
                assert np.array_equal(sc.cpu().numpy(), z[key + "/sc"]), key
                assert np.array_equal(vals.cpu().numpy(), z[key + "/vals"]), key
                if ref is None:
                    assert np.array_equal(pts.cpu().numpy(), z[key + "/pts"]), key
                else:
                    rough = z[key.replace("integral", "none") + "/pts"]
                    tol = _refine_tol(cms, torch.from_numpy(rough), sb.cpu().long() * cms.shape[1] + sc.cpu().long())
                    # (+ a relative term: an ill-conditioned patch also inflates the offset itself)
                    assert (np.abs(pts.cpu().numpy() - z[key + "/pts"]) <= tol + 1e-4 * np.abs(z[key + "/pts"])).all(), key
            else:
                ref = None if parts[1] == "none" else "integral"
                pts, vals = HP.find_global_peaks(cms, float(parts[2]), ref, 5)
                assert np.array_equal(vals.cpu().numpy(), z[key + "/vals"]), key
                if ref is None:
                    assert np.array_equal(pts.cpu().numpy(), z[key + "/pts"], equal_nan=True), key
                else:
                    rough = z[key.replace("integral", "none") + "/pts"].reshape(-1, 2)
                    ok = ~np.isnan(rough[:, 0])
                    tol = np.full((rough.shape[0], 1), 1e-5)
                    tol[ok] = _refine_tol(cms, torch.from_numpy(rough[ok]), torch.nonzero(torch.from_numpy(ok)).flatten())
                    d = np.abs(pts.cpu().numpy().reshape(-1, 2) - z[key + "/pts"].reshape(-1, 2))
                    assert (np.isnan(d) == np.isnan(rough)).all() and (np.nan_to_num(d) <= tol + 1e-4 * np.abs(np.nan_to_num(z[key + "/pts"].reshape(-1, 2)))).all(), key
            n_checked += 1
    assert n_checked >= 20


def test_local_peaks_capacity_retry_and_empty():
    from sleap_nn_amd.inference.ops import peaks as HP

    g = torch.Generator().manual_seed(1)
    cms = torch.rand((2, 3, 64, 64), generator=g)
    ref = O.find_local_peaks(cms, 0.2, "integral", 5)
    xy, vals, sb, sc, counts, _ = HP.find_local_peaks_device(cms.to(DEV), 0.2, "integral", 5, capacity=16)
    assert int(counts[0]) == ref[0].shape[0] > 16  # overflow is reported, not hidden
    pts, vals, sb, sc = HP.find_local_peaks(cms.to(DEV), 0.2, "integral", 5)  # retries internally
    assert np.array_equal(sc.cpu().numpy(), ref[3].numpy()) and np.array_equal(vals.cpu().numpy(), ref[1].numpy())
    assert np.allclose(pts.cpu().numpy(), ref[0].numpy(), atol=1e-5)
    e = HP.find_local_peaks(torch.zeros((1, 2, 8, 8), device=DEV), 0.2, "integral", 5)
    assert e[0].shape == (0, 2) and e[1].shape == (0,)


def _raw_local_peaks(cms, thr, refine, patch, cap, scratch_ints):
    """ph_local_peaks through the raw C ABI with a caller-chosen scratch size: the minimum runs the three-pass kernels, ph_local_peaks_scratch_bytes the one-pass pair."""
    import ctypes as C

    from sleap_nn_amd import _lib as L

    B, Cc, H, W = cms.shape
    xy = torch.full((cap, 2), -7.0, device=DEV)
    vals = torch.full((cap,), -7.0, device=DEV)
    sb = torch.full((cap,), -7, dtype=torch.int32, device=DEV)
    sc = torch.full((cap,), -7, dtype=torch.int32, device=DEV)
    counts = torch.zeros((2 + 2 * B,), dtype=torch.int32, device=DEV)
    scratch = torch.empty((scratch_ints,), dtype=torch.int32, device=DEV)
    with torch.cuda.device(DEV):
        L.check(L.lib().ph_local_peaks(C.c_void_p(cms.data_ptr()), B, Cc, H, W, float(thr), int(refine), patch, C.c_void_p(xy.data_ptr()), C.c_void_p(vals.data_ptr()), C.c_void_p(sb.data_ptr()),
                                       C.c_void_p(sc.data_ptr()), C.c_void_p(counts.data_ptr()), cap, 1.0, C.c_void_p(scratch.data_ptr()), scratch.numel() * 4, L.current_stream_ptr()))
    torch.cuda.synchronize()
    n = int(counts[0])
    return xy[: min(n, cap)].cpu(), vals[: min(n, cap)].cpu(), sb[: min(n, cap)].cpu(), sc[: min(n, cap)].cpu(), counts.cpu()


@pytest.mark.parametrize("shape,thr", [((2, 5, 37, 70), 0.5), ((1, 13, 64, 256), 0.2), ((3, 2, 19, 300), 0.6), ((1, 3, 24, 510), 0.3), ((2, 64, 16, 40), 0.7), ((1, 2, 40, 96), -1.0),
                                       ((1, 65, 16, 32), 0.5), ((1, 2, 8, 600), 0.5)])
def test_one_pass_local_peaks_equal_the_three_pass_kernels_and_the_oracle(shape, thr):
    """peaks_onepass_kernel + peaks_place_kernel (maps read once, two launches) against the three-pass kernels through the same C entry point and against the oracle:
    identical peak lists bit for bit -- order (sample, y, x, channel), values, refined coordinates, counts and offsets.  Cases: heights that are no multiple of the
    eight-row groups, widths in both column-chunk classes (<= 256, <= 512), with and without 16-byte-aligned rows, 64 channels (the mask width), a threshold below every value on noise (thousands of
    peaks per block: the staging area overflows and the placement pass recomputes those blocks), ties / plateaus (strict comparison), NaN entries, capacity overflow reporting;
    65 channels and 600 columns are outside the one-pass path (its scratch size equals the minimum) and must still work."""
    from sleap_nn_amd import _lib as L

    B, Cc, H, W = shape
    g = torch.Generator().manual_seed(H * W + Cc)
    cms = torch.rand(shape, generator=g)
    cms[:, :, H // 2, : W // 2] = torch.round(cms[:, :, H // 2, : W // 2] * 4) / 4  # ties along a row
    cms[0, 0, 0, 0] = cms[0, 0, H - 1, W - 1] = 2.0  # corners
    cms[0, 0, 3:5, 9:11] = 3.0  # a plateau: no strict maximum
    cms[-1, -1, 1, 2] = cms[0, 0, H - 1, 5] = float("nan")  # a NaN is no peak and neither is any pixel next to it (`v > NaN` is false; peaks.py's dilation propagates it)
    ref = O.find_local_peaks(cms, thr, "integral", 5)
    n_ref = ref[0].shape[0]
    dev = cms.to(DEV)
    min_ints = 2 * B * H + 2
    full_ints = int(L.lib().ph_local_peaks_scratch_bytes(B, Cc, H, W)) // 4
    assert (full_ints > min_ints) == (Cc <= 64 and W <= 512)
    cap = n_ref + 5
    three = _raw_local_peaks(dev, thr, 1, 5, cap, min_ints)
    one = _raw_local_peaks(dev, thr, 1, 5, cap, full_ints)
    for a, b_ in zip(three, one):  # (a refinement window that holds the NaN gives NaN coordinates in both)
        assert torch.equal(torch.nan_to_num(a.float(), nan=-123.0), torch.nan_to_num(b_.float(), nan=-123.0))
    xy, vals, sb, sc, counts = one
    assert int(counts[0]) == n_ref and int(counts[1 + 2 * B]) == n_ref
    assert np.array_equal(sb.numpy(), ref[2].numpy()) and np.array_equal(sc.numpy(), ref[3].numpy()) and np.array_equal(vals.numpy(), ref[1].numpy())
    assert np.allclose(xy.numpy(), ref[0].numpy(), atol=1e-4, equal_nan=True)
    per_sample = np.bincount(ref[2].numpy(), minlength=B)
    assert np.array_equal(counts[1 : 1 + B].numpy(), per_sample) and np.array_equal(counts[1 + B : 1 + 2 * B].numpy(), np.concatenate([[0], np.cumsum(per_sample)[:-1]]))
    small = _raw_local_peaks(dev, thr, 1, 5, max(n_ref // 2, 1), full_ints)  # output capacity too small: the count is still the truth, the rows that fit are right
    assert int(small[4][0]) == n_ref and torch.equal(small[1], vals[: small[1].shape[0]])


def test_one_pass_local_peaks_on_row_item_lane_and_chunk_boundaries():
    """The one-pass kernel drops values that lose against a neighbour its WAVE holds before they reach the candidate list (a 3x3 maximum formed in registers: rows of a
    four-row item, columns of the lane's quad and of the two neighbour lanes); what the wave does not hold must count as unknown, never as smaller.  Smooth blobs -- the
    shape the filter is made for -- centred ON every such boundary (rows 3|4 of an item, 7|8 of a block, columns 3|4 of a lane, 255|256 of a column chunk, the image
    border), pairs of EQUAL values facing each other across each of them (no strict maximum: no peak on either side), and a larger value just across a boundary from a
    would-be peak: the list must equal the oracle's, bit for bit, with and without 16-byte-aligned rows."""
    from sleap_nn_amd import _lib as L

    for W in (520 - 8, 300, 259):  # two column chunks (aligned), two chunks (W a multiple of 4), one odd width
        H, Cc = 29, 3
        yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
        cms = torch.zeros((2, Cc, H, W))
        centres = [(3, 3), (4, 4), (7, 20), (8, 31), (15, 32), (16, 255), (12, 256), (11, 257), (0, 100), (H - 1, 64), (20, 0), (23, W - 1), (24, 128), (19, 127), (3, 200), (4, 231)]
        for i, (cy, cx) in enumerate(centres):
            if cx < W:
                cms[i % 2, i % Cc] += (0.5 + 0.02 * i) * torch.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * 1.25**2))
        ties = [((3, 40), (4, 40)), ((7, 50), (8, 50)), ((10, 63), (10, 64)), ((13, 255), (13, 256)), ((3, 67), (4, 68)), ((7, 71), (8, 72)), ((20, 255), (21, 256)), ((26, 3), (26, 4))]
        for (y0, x0), (y1, x1) in ties:
            if max(x0, x1) < W:
                cms[1, 2, y0, x0] = cms[1, 2, y1, x1] = 0.9
        for (y0, x0), (y1, x1) in (((11, 80), (12, 80)), ((15, 83), (16, 84)), ((22, 87), (22, 88)), ((18, 255), (18, 256))):  # a larger value right across the boundary
            if max(x0, x1) < W:
                cms[0, 1, y0, x0], cms[0, 1, y1, x1] = 0.7, 0.8
        ref = O.find_local_peaks(cms, 0.2, "integral", 5)
        n_ref = ref[0].shape[0]
        assert n_ref > 15
        dev = cms.to(DEV)
        full_ints = int(L.lib().ph_local_peaks_scratch_bytes(2, Cc, H, W)) // 4
        assert full_ints > 2 * 2 * H + 2
        xy, vals, sb, sc, counts = _raw_local_peaks(dev, 0.2, 1, 5, n_ref + 8, full_ints)
        assert int(counts[0]) == n_ref
        assert np.array_equal(sb.numpy(), ref[2].numpy()) and np.array_equal(sc.numpy(), ref[3].numpy()) and np.array_equal(vals.numpy(), ref[1].numpy())
        assert np.allclose(xy.numpy(), ref[0].numpy(), atol=1e-4, equal_nan=True)
        three = _raw_local_peaks(dev, 0.2, 1, 5, n_ref + 8, 2 * 2 * H + 2)
        for a, b_ in zip(three, (xy, vals, sb, sc, counts)):
            assert torch.equal(a, b_)


@pytest.mark.parametrize("name", ["chain5", "tree6", "chain13", "rev4"])
def test_paf_scoring_and_grouping_match_reference(name):
    from sleap_nn_amd.inference.ops.paf import PAFScorer
    from sleap_nn_amd.inference.ops.peaks import find_local_peaks

    z = G.load("paf.npz")
    meta = json.loads(str(z["meta_json"]))["specs"][name]
    edges = [tuple(e) for e in meta["edges"]]
    n_nodes = meta["n_nodes"]
    names = [f"n{i}" for i in range(n_nodes)]
    sc = PAFScorer(names, [(names[s], names[d]) for s, d in edges], meta["pafs_stride"])
    assert list(sc.sorted_edge_inds) == z[f"{name}/sorted_edge_inds"].tolist()
    cms = torch.from_numpy(z[f"{name}/cms"]).to(DEV)
    pafs = torch.from_numpy(z[f"{name}/pafs"]).to(DEV)
    pts, vals, sb, ch = find_local_peaks(cms, 0.2, "integral", 5)
    pts = pts * meta["cms_stride"]
    B = cms.shape[0]
    pk = [pts[sb == b] for b in range(B)]
    pv = [vals[sb == b] for b in range(B)]
    pc = [ch[sb == b] for b in range(B)]
    inst, ivals, iscores, e, p, s = sc.predict(pafs.permute(0, 2, 3, 1), pk, pv, pc)
    for b in range(B):
        re_, rp_, rs_ = (G.ragged(z, f"{name}/{k}")[b] for k in ("edge_inds", "edge_peak_inds", "line_scores"))
        pe, pp, ps = e[b].cpu().numpy(), p[b].cpu().numpy(), s[b].cpu().numpy()
        ob = np.lexsort((rp_[:, 1], rp_[:, 0], re_))  # reference order inside an edge is machine dependent
        assert np.array_equal(pe, re_[ob]) and np.array_equal(pp, rp_[ob])
        assert np.allclose(ps, rs_[ob], atol=2e-6, equal_nan=True)
        ref = G.ragged(z, f"{name}/inst")[b].reshape(-1, n_nodes, 2)
        got = inst[b].numpy()
        assert got.shape == ref.shape
        assert np.array_equal(np.isnan(got), np.isnan(ref))  # grouping membership bit-exact
        assert np.allclose(got, ref, atol=1e-4, equal_nan=True)
        assert np.array_equal(np.nan_to_num(ivals[b].numpy()), np.nan_to_num(G.ragged(z, f"{name}/inst_vals")[b]))
        assert np.allclose(iscores[b].numpy(), G.ragged(z, f"{name}/inst_scores")[b], atol=1e-5)


def test_line_sampling_bit_exact_on_awkward_coordinates():
    """Round-half-even, negative coordinates and clipping (paf.py:177-234 vector from the reference)."""
    from sleap_nn_amd.inference.ops.paf import PAFScorer

    z = G.load("paf.npz")
    pk = torch.from_numpy(z["linesubs/peaks"])
    out = z["linesubs/out"]  # (n, 10, 2, 3) rows, cols, channel
    H, W = 12, 6
    # a PAF whose value encodes its own (row, col): x-channel = row*W+col, y-channel = 0
    base = torch.arange(H * W, dtype=torch.float32).reshape(H, W)
    # build one sample per candidate pair so that each pair is the only candidate of edge 0
    epi = z["linesubs/epi"]
    sc = PAFScorer(["a", "b"], [("a", "b")], pafs_stride=2, max_edge_length_ratio=1e9)
    for i in range(epi.shape[0]):
        s, d = int(epi[i, 0]), int(epi[i, 1])
        if s == d:
            continue
        pafs = torch.zeros((1, 2, H, W))
        pafs[0, 0] = base
        peaks = [torch.stack([pk[s], pk[d]]).to(DEV)]
        ch = [torch.tensor([0, 1], dtype=torch.int32, device=DEV)]
        _, _, ls = sc.score_paf_lines(pafs.to(DEV).permute(0, 2, 3, 1), peaks, ch)
        vec = pk[d] - pk[s]
        ux = float(vec[0] / torch.norm(vec))
        expect = np.mean([float(base[out[i, k, 0, 0], out[i, k, 0, 1]]) * ux for k in range(10)])
        assert abs(float(ls[0][0]) - expect) <= 1e-4 * max(1.0, abs(expect)), (i, float(ls[0][0]), expect)


def _bottomup_layer(cfg, weights, **kw):
    from sleap_nn_amd.inference.backends import HipBackend
    from sleap_nn_amd.inference.layers import BottomUpLayer, PostprocessConfig
    from sleap_nn_amd.inference.ops.paf import PAFScorer

    m = _model(cfg, weights)
    hc = cfg["heads"]
    sc = PAFScorer.from_config(hc)
    return BottomUpLayer(HipBackend(m, DEV), sc, hc["confmaps"]["output_stride"], hc["pafs"]["output_stride"], max_stride=cfg["backbone"]["max_stride"], **kw)


def test_bottomup_layer_reproduces_reference_golden():
    """End to end on the reference's own fixture checkpoint + golden frames
    (tests/inference/parity_golden/bottomup.pkl)."""
    z = G.load("ckpt_bottomup.npz")
    cfg = G.config(z)
    layer = _bottomup_layer(cfg, G.weights(z))
    out = layer.predict(torch.from_numpy(z["image"]).squeeze(1))
    k, v, s = out.pred_keypoints.numpy(), out.pred_peak_values.numpy(), out.instance_scores.numpy()
    gp, gv, gs = G.ragged(z, "gold_peaks"), G.ragged(z, "gold_vals"), G.ragged(z, "gold_scores")
    assert k.shape[0] == len(gp)
    for b in range(k.shape[0]):
        n = gp[b].shape[0]
        ref = gp[b].reshape(n, -1, 2)
        assert np.array_equal(np.isnan(k[b, :n]), np.isnan(ref))
        assert np.allclose(k[b, :n], ref, atol=1e-3, equal_nan=True)
        assert np.isnan(k[b, n:]).all()
        assert np.allclose(v[b, :n], gv[b], atol=CMS_ATOL, equal_nan=True)
        assert np.allclose(s[b, :n], gs[b], atol=1e-4)


def test_single_instance_layer_reproduces_reference_golden():
    from sleap_nn_amd.inference.backends import HipBackend
    from sleap_nn_amd.inference.layers import SingleInstanceLayer

    z = G.load("ckpt_single_instance.npz")
    cfg = G.config(z)
    m = _model(cfg, G.weights(z))
    hc = cfg["heads"]["confmaps"]
    layer = SingleInstanceLayer(HipBackend(m, DEV), hc["output_stride"], max_stride=cfg["backbone"]["max_stride"])
    out = layer.predict(torch.from_numpy(z["image"]).squeeze(1))
    # the golden was captured with input scale 0.5 (frames in the fixture are already scaled)
    k = out.pred_keypoints[:, 0].cpu().numpy() / cfg["preprocessing"]["scale"]
    assert np.allclose(k, z["gold_peaks"], atol=1e-3, equal_nan=True)
    assert np.allclose(out.pred_peak_values[:, 0].cpu().numpy(), z["gold_vals"], atol=CMS_ATOL)


def test_bottomup_vs_oracle_on_rendered_heads_full_size():
    """cfg3-sized post-process (13 nodes / 12 edges, 256x256 confmaps, 128x128 PAFs) vs the oracle."""
    from sleap_nn_amd.inference.layers.bottomup import BottomUpLayer
    from sleap_nn_amd.inference.ops.paf import PAFScorer
    from sleap_nn_amd.inference.preprocess_info import PreprocInfo

    n_nodes, size = 13, 1024
    edges = [(i, i + 1) for i in range(12)]
    names = [str(i) for i in range(n_nodes)]
    B = 3
    cms = torch.stack([O.render_confmaps(O.render_instances(size, n_nodes, 6, 777 + b), size, 4, 2.5 * 4 / 2) for b in range(B)])
    pafs = torch.stack([O.render_pafs(O.render_instances(size, n_nodes, 6, 777 + b), edges, size, 8, 30.0) for b in range(B)])
    ref_sc = O.PAFScorerRef(names, [(names[s], names[d]) for s, d in edges], 8)
    rk, rv, rs = O.bottomup_postprocess(cms, pafs, ref_sc, 4)

    class _NoBackend:
        device = DEV
        does_baked_postproc = False

        def __call__(self, x):
            raise AssertionError

        def warmup(self, s):
            pass

    layer = BottomUpLayer(_NoBackend(), PAFScorer(names, [(names[s], names[d]) for s, d in edges], 8), 4, 8)
    out = layer.postprocess({"MultiInstanceConfmapsHead": cms.to(DEV), "PartAffinityFieldsHead": pafs.to(DEV)}, PreprocInfo(eff_scale=torch.ones(B)))
    k = out.pred_keypoints.numpy()
    assert k.shape == rk.shape
    assert np.array_equal(np.isnan(k), np.isnan(rk))
    assert np.allclose(k, rk, atol=1e-4, equal_nan=True)
    assert np.array_equal(np.nan_to_num(out.pred_peak_values.numpy()), np.nan_to_num(rv))
    assert np.allclose(out.instance_scores.numpy(), rs, atol=1e-5, equal_nan=True)


def test_max_instances_and_skip_guard():
    z = G.load("ckpt_bottomup.npz")
    cfg = G.config(z)
    img = torch.from_numpy(z["image"]).squeeze(1)
    layer = _bottomup_layer(cfg, G.weights(z), max_instances=1)
    out = layer.predict(img)
    assert out.pred_keypoints.shape[1] == 1
    full = _bottomup_layer(cfg, G.weights(z)).predict(img)
    best = np.nanargmax(full.instance_scores.numpy(), axis=1)
    for b in range(img.shape[0]):
        assert np.allclose(out.pred_keypoints[b, 0].numpy(), full.pred_keypoints[b, best[b]].numpy(), equal_nan=True)
    skip = _bottomup_layer(cfg, G.weights(z), max_peaks_per_node=0).predict(img)
    assert np.isnan(skip.pred_keypoints.numpy()).all()


def test_cfg3_network_vs_oracle_one_frame():
    """The bench network (7.8 M params) on a 256x256 crop: confmaps/PAFs within 1e-4 of the oracle."""
    from sleap_nn_amd.architectures.model import Model

    bb = {"in_channels": 1, "kernel_size": 3, "filters": 16, "filters_rate": 2, "max_stride": 32, "stem_stride": None, "middle_block": True, "up_interpolate": True, "stacks": 1, "convs_per_block": 2, "output_stride": 4}
    heads = {"confmaps": {"part_names": [str(i) for i in range(13)], "output_stride": 4}, "pafs": {"edges": [[str(i), str(i + 1)] for i in range(12)], "output_stride": 8}}
    sd = O.init_state(bb, heads, "bottomup")
    m = Model("unet", bb, heads, "bottomup")
    m.load_state_dict(sd)
    g = torch.Generator().manual_seed(4321)
    img = torch.randint(0, 256, (2, 1, 256, 256), dtype=torch.uint8, generator=g)
    ref = O.model_forward(sd, bb, heads, "bottomup", img)
    out = m.to(DEV)(img.to(DEV))
    for k, v in ref.items():
        _head_close(out[k], v, k)


_CFG3_REF = {}


@pytest.mark.parametrize("precision", ["exact", "split"])
def test_cfg3_benched_workload_full_size_vs_oracle_and_batch_invariance(precision):
    """The workload bench.py times -- cfg3 network, bench.py's own weights (xavier seed 1234, heads x0.05), 1024x1024 uint8
    frames -- under parity at FULL size with DEFAULT options at every per-rank batch the bench's scaling runs use (32 / 8 / 4 frames, and 2 / 1):
    two frames against the oracle (confmaps / PAFs within 1e-4 and 1e-5 of the head's scale); then, with the kernel choice pinned to the list the
    default 32-frame forward took, frame 0 of a 32-frame launch bit-identical to the same frame launched alone (persistent-workgroup tile walk, XCD
    dealing and workspace offsets all change with the batch; the arithmetic per output must not)."""
    import bench
    from sleap_nn_amd.architectures.model import Model

    m = Model("unet", bench.CFG3_BB, bench.CFG3_HEADS, "bottomup").init_xavier_(seed=1234, head_scale=0.05).to(DEV).set_precision(precision)
    sd = m.state_dict()
    g = torch.Generator().manual_seed(4321)
    frames = torch.randint(0, 256, (32, 1, bench.SIZE, bench.SIZE), dtype=torch.uint8, generator=g)
    ref = _CFG3_REF.get("ref")
    if ref is None:
        ref = _CFG3_REF["ref"] = O.model_forward(sd, bench.CFG3_BB, bench.CFG3_HEADS, "bottomup", frames[:2])
    dev_frames = frames.to(DEV)
    # (1) What bench.py runs: DEFAULT options.  Which kernel takes a layer depends on the number of work units to deal over the CUs, i.e. on the batch
    # (conv3x3_route: F(4x4,3x3) vs F(2x2,3x3) by rounds of the chip; K split over workgroups when a layer fills less than half of them), so every
    # per-rank batch of the bench's scaling runs is put under parity with the routing IT takes: 32 frames (N = 1), 8 (4 GPUs), 4 (8 GPUs), and 2 / 1.
    default_kernels = {}
    for nb in (32, 8, 4, 2, 1):
        out = m(dev_frames[:nb].contiguous())
        default_kernels[nb] = m.last_kernels()
        for k, v in ref.items():
            _head_close(out[k][: min(nb, 2)], v[: min(nb, 2)], (k, nb))  # these heads are O(1e-3): relative bar as well
            assert torch.isfinite(out[k]).all()
    if precision == "exact":
        from sleap_nn_amd import _lib as L

        assert L.KV_WINO4 in default_kernels[32] and L.KV_WINO2D_KS not in default_kernels[32]
        assert L.KV_SMALLMAP in default_kernels[1] or L.KV_WINO2D_KS in default_kernels[1]  # the one-frame launch is in the small-batch regime (conv3x3_sm_kernel / split K)
    # (2) Bit-for-bit batch invariance is a property of ONE kernel choice, so the choice is pinned -- F(4x4,3x3) wherever the shape fits and no split K:
    # exactly the kernel list the default 32-frame forward took (asserted), i.e. the benched kernels are the ones compared bit by bit.
    m.set_option("conv_wino4", 3)
    m.set_option("conv_splitk", 0)
    out2 = {k: v.clone() for k, v in m(dev_frames[:2].contiguous()).items()}
    for k, v in ref.items():
        _head_close(out2[k], v, k)
    one = {k: v.clone() for k, v in m(dev_frames[:1].contiguous()).items()}
    full = m(dev_frames)
    assert m.last_kernels() == default_kernels[32], (m.last_kernels(), default_kernels[32])
    torch.cuda.synchronize()
    for k in one:
        assert torch.equal(full[k][:1], one[k]), k
        assert torch.equal(full[k][:2], out2[k]), k
        assert torch.isfinite(full[k]).all()


# ------------------------------------------------------------------------------------------
# fp16-matrix-pipe precisions (Model.set_precision): "split" = every operand a (hi, lo) pair of fp16 numbers, three MFMAs per
# product, fp32 accumulation -- must meet the SAME 1e-4 bar as the exact path; "fp16" = the reference's autocast mode, whose
# own tolerance is 5e-3 (reference tests/inference/test_cuda.py:54-55).
# ------------------------------------------------------------------------------------------
FP16_ATOL = 5e-3


@pytest.mark.parametrize("name", ["unet_tiny_interp.npz", "unet_tiny_trans.npz", "unet_tiny_bu13.npz", "unet_tiny_rgb.npz", "ckpt_bottomup.npz", "ckpt_single_instance.npz", "unet_f16_wino.npz"]
                         + CPB_GOLDENS)
@pytest.mark.parametrize("precision,atol", [("split", CMS_ATOL), ("fp16", FP16_ATOL)])
def test_forward_matches_reference_golden_on_the_fp16_pipe(name, precision, atol):
    """All six reference goldens (bilinear and transposed-conv decoders, RGB input, the two fixture checkpoints) through the
    fp16-pipe kernels, head outputs AND the intermediate activations that exist in HBM (read back from the split / fp16
    activation formats)."""
    z = G.load(name)
    cfg = G.config(z)
    m = _model(cfg, G.weights(z)).set_precision(precision).set_keep_activations(True)
    out = m(torch.from_numpy(z["image"]).squeeze(1).to(DEV))
    torch.cuda.synchronize()
    assert m.get_option("conv_precision") == {"split": 1.0, "fp16": 2.0}[precision]
    for k in [f for f in z.files if f.startswith("out/")]:
        err = (out[k[4:]].cpu() - torch.from_numpy(z[k])).abs().max().item()
        assert err <= atol, (k, err)
    n_act = 0
    found = []
    for k in [f for f in z.files if f.startswith("act/")]:
        ref = torch.from_numpy(z[k])
        try:
            got = m.read_activation(k[4:], ref.shape[0], ref.shape[-2:]).cpu()
        except KeyError:
            continue
        assert (got - ref).abs().max().item() <= atol * max(1.0, ref.abs().max().item()), k
        n_act += 1
        found.append(k[4:])
    assert n_act >= 2 or not any(f.startswith("act/") for f in z.files)
    _assert_block_structure_activations_found(name, cfg, found)


def test_split_precision_is_fp32_equivalent_on_the_benched_network():
    """cfg3 network at 256x384 with O(1) head outputs (head_scale 1): the split-fp16 path must be as close to the oracle as
    the exact-fp32 path is (within 2x of its error, both far inside 1e-4), odd sizes and the unfused program included."""
    import bench
    from sleap_nn_amd.architectures.model import Model

    sd = O.init_state(bench.CFG3_BB, bench.CFG3_HEADS, "bottomup", seed=11, head_scale=1.0)
    g = torch.Generator().manual_seed(5)
    img = torch.randint(0, 256, (3, 1, 256, 384), dtype=torch.uint8, generator=g)
    ref = O.model_forward(sd, bench.CFG3_BB, bench.CFG3_HEADS, "bottomup", img)
    errs = {}
    for prec in ("exact", "split"):
        m = Model("unet", bench.CFG3_BB, bench.CFG3_HEADS, "bottomup")
        m.load_state_dict(sd)
        out = m.to(DEV).set_precision(prec)(img.to(DEV))
        errs[prec] = {k: (out[k].cpu() - v).abs().max().item() / v.abs().max().item() for k, v in ref.items()}
    for k in ref:
        assert errs["split"][k] <= max(2.0 * errs["exact"][k], 2e-6), (k, errs)
        assert errs["split"][k] * ref[k].abs().max().item() <= CMS_ATOL


def test_fp16_pipe_odd_sizes_pool_padding_and_bitwise_determinism():
    """Odd feature-map sizes (the fused pool's zero padding, partial tiles) and a second launch on another stream in split precision."""
    from sleap_nn_amd.architectures.model import Model

    bb = {"in_channels": 1, "kernel_size": 3, "filters": 12, "filters_rate": 1.5, "max_stride": 8, "stem_stride": None, "middle_block": True, "up_interpolate": True,
          "stacks": 1, "convs_per_block": 2, "output_stride": 2}
    heads = {"confmaps": {"part_names": ["a", "b", "c"], "output_stride": 2}}
    sd = O.init_state(bb, heads, "single_instance", seed=3, head_scale=1.0)
    g = torch.Generator().manual_seed(6)
    img = torch.randint(0, 256, (2, 1, 104, 72), dtype=torch.uint8, generator=g)
    ref = O.model_forward(sd, bb, heads, "single_instance", img)["SingleInstanceConfmapsHead"]
    for prec, atol in (("split", CMS_ATOL), ("fp16", FP16_ATOL)):
        m = Model("unet", bb, heads, "single_instance")
        m.load_state_dict(sd)
        m.to(DEV).set_precision(prec)
        a = m(img.to(DEV))["SingleInstanceConfmapsHead"].clone()
        assert (a.cpu() - ref).abs().max().item() <= atol, prec
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            b = m(img.to(DEV))["SingleInstanceConfmapsHead"].clone()
        s.synchronize()
        assert torch.equal(a, b), prec


@pytest.mark.parametrize("hw,batch,nodes,out_stride", [((96, 128), 2, 17, 4), ((104, 72), 1, 5, 4), ((64, 160), 3, 32, 4), ((64, 64), 1, 33, 4)])
def test_head_fused_into_the_fp16_conv_epilogue_matches_the_head_kernel_and_the_oracle(hw, batch, nodes, out_stride):
    """Plain fp16 (autocast mode): the 1x1 head behind the last decoder conv of 64 channels (filters 16, output stride 4) as four v_mfma_f32_32x32x16_f16 on the conv kernel's staged
    fp16 row -- image-cut tiles, 1 .. 32 head channels (33: not fused, the head kernel runs), an inference plan (the conv's own output never reaches HBM) and a keep-everything plan;
    vs the separate head launch (head_fuse = 0: the same fp16-rounded activations, another summation order) and vs the oracle at the fp16 bar."""
    from sleap_nn_amd.architectures.model import Model
    from sleap_nn_amd import _lib as L

    bb = {"in_channels": 1, "kernel_size": 3, "filters": 16, "filters_rate": 2, "max_stride": 8, "stem_stride": None, "middle_block": True, "up_interpolate": True,
          "stacks": 1, "convs_per_block": 2, "output_stride": out_stride}
    heads = {"confmaps": {"part_names": [f"n{i}" for i in range(nodes)], "output_stride": out_stride}}
    sd = O.init_state(bb, heads, "single_instance", seed=nodes, head_scale=1.0)
    img = torch.randint(0, 256, (batch, 1, hw[0], hw[1]), dtype=torch.uint8, generator=torch.Generator().manual_seed(hw[1]))
    ref = O.model_forward(sd, bb, heads, "single_instance", img)["SingleInstanceConfmapsHead"]
    outs = {}
    for fuse, reuse in ((1, 1), (1, 0), (0, 1)):
        m = Model("unet", bb, heads, "single_instance")
        m.load_state_dict(sd)
        m.set_option("head_fuse", fuse).set_option("workspace_reuse", reuse)
        m.to(DEV).set_precision("fp16")
        outs[(fuse, reuse)] = m(img.to(DEV))["SingleInstanceConfmapsHead"].cpu()
        head_codes = [c for r, c in zip(m.op_table(batch, hw[0], hw[1]), m.last_kernels()) if r["kind"] == L.OP_HEAD]
        assert head_codes == [L.KV_FUSED if (fuse and nodes <= 32) else L.KV_NONE], (fuse, head_codes)
        assert torch.equal(m(img.to(DEV))["SingleInstanceConfmapsHead"].cpu(), outs[(fuse, reuse)])
    scale = ref.abs().max().item()
    assert (outs[(1, 1)] - ref).abs().max().item() <= FP16_ATOL
    assert torch.equal(outs[(1, 1)], outs[(1, 0)])  # the unread-output form stores nothing else
    assert (outs[(1, 1)] - outs[(0, 1)]).abs().max().item() <= 2e-6 * max(scale, 1.0)  # same fp16 operands, fp32 accumulation in another order


def test_training_module_keeps_exact_fp32_while_inference_runs_split():
    """A model set to "split" for inference switches to the exact fp32 program for training (the backward needs fp32
    activations) and back; ph_model_backward refuses activations of an fp16-pipe forward."""
    from sleap_nn_amd.architectures.model import Model

    z = G.load("unet_tiny_interp.npz")
    cfg = G.config(z)
    m = _model(cfg, G.weights(z)).set_precision("split")
    img = torch.from_numpy(z["image"]).squeeze(1).to(DEV)
    m(img)
    assert m.get_option("conv_precision") == 1.0
    m.train(True)
    m(img)
    assert m.get_option("conv_precision") == 0.0
    m.eval()
    m(img)
    assert m.get_option("conv_precision") == 1.0


def test_cfg5_multiclass_bottomup_768_fp16_network_and_full_size_postprocess():
    """BASELINE cfg5: multi-class bottom-up, 768x768, 4 classes x 17 keypoints, fp16 MFMA.  The reference has no HRNet
    (SURVEY section 0), so the backbone is its UNet; what cfg5 adds to the path is (1) the fp16 (autocast-equivalent) forward --
    head outputs incl. the sigmoid class maps within the reference's own fp16 tolerance 5e-3 of the fp32 oracle, and the
    keypoints it yields within 1e-3 px of the oracle's on the same maps -- and (2) the multi-class post-process at FULL
    size: 16 frames of (17, 192, 192) confidence maps + (4, 96, 96) class maps, identical to the oracle's."""
    import bench
    from sleap_nn_amd.architectures.model import Model
    from sleap_nn_amd.inference.backends import HipBackend
    from sleap_nn_amd.inference.layers import BottomUpMultiClassLayer, PostprocessConfig
    from sleap_nn_amd.inference.preprocess_info import PreprocInfo

    S, N, K = 768, 17, 4
    names = [f"k{i}" for i in range(N)]
    heads = {"confmaps": {"part_names": names, "sigma": 2.5, "output_stride": 4, "loss_weight": 1.0},
             "class_maps": {"classes": [f"id{i}" for i in range(K)], "sigma": 12.5, "output_stride": 8, "loss_weight": 1.0}}
    bb = dict(bench.CFG3_BB)
    sd = O.init_state(bb, heads, "multi_class_bottomup", seed=17, head_scale=1.0)
    g = torch.Generator().manual_seed(55)
    img = torch.randint(0, 256, (2, 1, S, S), dtype=torch.uint8, generator=g)
    ref = O.model_forward(sd, bb, heads, "multi_class_bottomup", img)
    m = Model("unet", bb, heads, "multi_class_bottomup")
    m.load_state_dict(sd)
    backend = HipBackend(m, DEV, use_fp16=True)  # TorchBackend(use_fp16=True) counterpart
    raw = backend(img)
    assert m.get_option("conv_precision") == 2.0 and all(v.dtype == torch.float32 for v in raw.values())
    for k, v in ref.items():
        err = (raw[k].cpu() - v).abs().max().item()
        assert err <= FP16_ATOL * max(1.0, v.abs().max().item()), (k, err, v.abs().max().item())
        # ... and band by band (eight output rows against that band's own scale): a corrupted halo line of one persistent tile cannot hide behind the head's global maximum
        d = (raw[k].cpu() - v).abs()
        bands = lambda t: t.reshape(t.shape[0], t.shape[1], t.shape[2] // 8, 8, t.shape[3]).amax(dim=(1, 3, 4))  # noqa: E731 (192 and 96 rows: whole bands)
        band_err, band_scale = bands(d), bands(v.abs()).clamp(min=1.0)
        print(f"cfg5 fp16 vs oracle, {k}: worst band {(band_err / band_scale).max().item():.3e} of its scale (bar {FP16_ATOL})")
        assert (band_err <= FP16_ATOL * band_scale).all(), (k, (band_err / band_scale).max().item())

    # ---- full-size post-process on rendered heads: 16 frames, 4 animals (one per class), 17 nodes
    B = 16
    rng = np.random.RandomState(3)
    pts = np.stack([np.clip(rng.uniform(120, S - 120, size=(K, 1, 2)) + rng.normal(0, 35, size=(K, N, 2)), 6, S - 7) for _ in range(B)]).astype(np.float32)
    cms = torch.stack([O.render_confmaps(pts[b], S, 4, 2.5 * 4 / 2) for b in range(B)])
    yy, xx = torch.meshgrid(torch.arange(0, S, 8, dtype=torch.float32), torch.arange(0, S, 8, dtype=torch.float32), indexing="ij")
    cmaps = torch.zeros(B, K, S // 8, S // 8)
    for b in range(B):
        for k in range(K):  # a class map = blobs (sigma 50 px) around that animal's nodes (data/identity.py:34-85 semantics)
            d2 = (xx[None] - torch.from_numpy(pts[b, k, :, 0])[:, None, None]) ** 2 + (yy[None] - torch.from_numpy(pts[b, k, :, 1])[:, None, None]) ** 2
            cmaps[b, k] = torch.exp(-d2 / (2 * 50.0**2)).amax(0)
    layer = BottomUpMultiClassLayer(backend, 4, 8, max_stride=32, postprocess_config=PostprocessConfig(peak_threshold=0.2))
    out = layer.postprocess({"MultiInstanceConfmapsHead": cms.to(DEV), "ClassMapsHead": cmaps.to(DEV)}, PreprocInfo(eff_scale=torch.ones(B)))
    rk, rv, rs, rt = O.multiclass_postprocess(cms, cmaps, 4, 8, peak_threshold=0.2)
    k = out.pred_keypoints.numpy()
    assert k.shape == tuple(rk.shape) == (B, K, N, 2)
    assert np.array_equal(np.isnan(k), np.isnan(rk.numpy()))
    assert int((~np.isnan(k[..., 0])).sum()) >= 0.9 * B * K * N  # nearly every rendered keypoint is found and assigned
    assert np.allclose(k, rk.numpy(), atol=1e-4, equal_nan=True)
    assert np.array_equal(np.nan_to_num(out.pred_peak_values.numpy()), np.nan_to_num(rv.numpy()))  # peak values bit-exact
    assert np.allclose(out.instance_scores.numpy(), rs.numpy(), atol=1e-6, equal_nan=True)
    assert np.allclose(out.instance_tracking_scores.numpy(), rt.numpy(), atol=1e-6, equal_nan=True)


def test_transposed_conv_phase_gemms_equal_zero_stuffing_and_carry_epilogue_parameters():
    """(1) The four output-phase GEMMs of ConvTranspose2d(k3, s2, p1, op1) against the zero-stuff + 3x3-conv formulation
    (handle option convt_phase = 0) and the reference golden, odd input sizes included.  (2) The activation and a folded
    BatchNorm are epilogue parameters of those GEMMs (north_star's "ConvTranspose + BN + SiLU decoder stage"; the reference
    builds its decoder with batch_norm=False + ReLU): a hand-built op program through the C ABI vs torch."""
    import ctypes as C

    import torch.nn.functional as F

    from sleap_nn_amd import _lib as L

    z = G.load("unet_tiny_trans.npz")
    cfg = G.config(z)
    img = torch.from_numpy(z["image"]).squeeze(1)[:, :, :40, :56].contiguous().to(DEV)  # 5x7 maps at the deepest level
    outs = {}
    for phase in (1, 0):
        m = _model(cfg, G.weights(z)).set_option("convt_phase", phase)
        outs[phase] = {k: v.clone() for k, v in m(img).items()}
    ref = O.model_forward(G.weights(z), cfg["backbone"], cfg["heads"], cfg["model_type"], img.cpu())
    for k, v in ref.items():
        assert (outs[1][k].cpu() - v).abs().max().item() <= CMS_ATOL
        assert (outs[1][k] - outs[0][k]).abs().max().item() <= 2e-5

    # ---- hand-built program: image -> conv3x3(1 -> 24) + ReLU -> ConvT(24 -> 40) * scale + shift -> SiLU -> head 1x1 (40 -> 3)
    lib = L.lib()
    g = torch.Generator().manual_seed(8)
    w0, b0 = torch.randn(24, 1, 3, 3, generator=g) * 0.3, torch.randn(24, generator=g) * 0.1
    wt, bt = torch.randn(24, 40, 3, 3, generator=g) * 0.1, torch.randn(40, generator=g) * 0.1
    sc, sh = torch.rand(40, generator=g) + 0.5, torch.randn(40, generator=g) * 0.2
    wh, bh = torch.randn(3, 40, 1, 1, generator=g) * 0.2, torch.randn(3, generator=g) * 0.1
    tensors = [t.contiguous() for t in (w0, b0, wt, bt, sc, sh, wh, bh)]
    ops = (L.OpDesc * 3)()
    for i, (kind, src0, dst, cin0, cout, ks, flags, w, b, w2, b2, oi) in enumerate([
        (L.OP_INPUT_CONV, -1, 0, 1, 24, 3, L.FLAG_RELU, 0, 1, -1, -1, -1),
        (L.OP_CONVT, 0, 1, 24, 40, 3, L.FLAG_SILU, 2, 3, 4, 5, -1),
        (L.OP_HEAD, 1, -1, 40, 3, 1, 0, 6, 7, -1, -1, 0),
    ]):
        d = ops[i]
        d.kind, d.src0, d.src1, d.dst, d.cin0, d.cin1, d.cout, d.ksize, d.flags = kind, src0, -1, dst, cin0, 0, cout, ks, flags
        d.weight, d.bias, d.out_index, d.dst2, d.weight2, d.bias2, d.cmid = w, b, oi, -1, w2, b2, 0
    ptrs = (C.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])
    numel = (C.c_int64 * len(tensors))(*[t.numel() for t in tensors])
    with torch.cuda.device(DEV):
        h = C.c_void_p(lib.ph_model_create(ops, 3, ptrs, numel, len(tensors), 2, 1))
        assert h, lib.ph_last_error()
        x = torch.randint(0, 256, (2, 1, 21, 34), dtype=torch.uint8, generator=g)
        xd = x.to(DEV)
        need = L.check(lib.ph_model_workspace_bytes(h, 2, 21, 34))
        ws = torch.empty(int(need), dtype=torch.uint8, device=DEV)
        out = torch.empty((2, 3, 42, 68), dtype=torch.float32, device=DEV)
        optr = (C.c_void_p * 1)(out.data_ptr())
        L.check(lib.ph_model_forward(h, C.c_void_p(xd.data_ptr()), 0, 2, 1, 21, 34, C.c_void_p(ws.data_ptr()), ws.numel(), optr, L.current_stream_ptr()))
        torch.cuda.synchronize()
        lib.ph_model_destroy(h)
    y = F.relu(F.conv2d(x.float() / 255.0, w0, b0, padding=1))
    y = F.conv_transpose2d(y, wt, bt, stride=2, padding=1, output_padding=1)
    y = F.silu(y * sc.view(1, -1, 1, 1) + sh.view(1, -1, 1, 1))  # BatchNorm2d.eval() folded to scale / shift, then SiLU
    y = F.conv2d(y, wh, bh)
    assert (out.cpu() - y).abs().max().item() <= CMS_ATOL


def test_cfg2_single_instance_512_network_and_full_size_global_peaks():
    """BASELINE cfg2 at full size: single-instance UNet f16/r2/max_stride 16/output_stride 2, 512x512, 13 keypoints, batch 8.
    Network: two frames vs the oracle (1e-4).  Post-process at the full (8, 13, 256, 256) size on rendered single-animal maps plus
    engineered ties (global-peak x / y are taken independently, first maximum each: SURVEY Q5): coordinates and values vs the oracle."""
    from sleap_nn_amd.architectures.model import Model
    from sleap_nn_amd.inference.backends import HipBackend
    from sleap_nn_amd.inference.layers import SingleInstanceLayer
    from sleap_nn_amd.inference.preprocess_info import PreprocInfo

    S, N, B = 512, 13, 8
    bb = {"in_channels": 1, "kernel_size": 3, "filters": 16, "filters_rate": 2, "max_stride": 16, "stem_stride": None, "middle_block": True, "up_interpolate": True,
          "stacks": 1, "convs_per_block": 2, "output_stride": 2}
    heads = {"confmaps": {"part_names": [f"k{i}" for i in range(N)], "sigma": 2.5, "output_stride": 2, "loss_weight": 1.0}}
    sd = O.init_state(bb, heads, "single_instance", seed=2, head_scale=1.0)
    g = torch.Generator().manual_seed(77)
    img = torch.randint(0, 256, (B, 1, S, S), dtype=torch.uint8, generator=g)
    m = Model("unet", bb, heads, "single_instance")
    m.load_state_dict(sd)
    layer = SingleInstanceLayer(HipBackend(m, DEV), 2, max_stride=16)
    raw = layer.backend(img)["SingleInstanceConfmapsHead"]
    ref = O.model_forward(sd, bb, heads, "single_instance", img[:2])["SingleInstanceConfmapsHead"]
    assert tuple(raw.shape) == (B, N, 256, 256)
    _head_close(raw[:2], ref, "cfg2")
    rng = np.random.RandomState(4)
    pts = np.stack([np.clip(rng.uniform(120, S - 120, size=(1, 1, 2)) + rng.normal(0, 45, size=(1, N, 2)), 4, S - 5) for _ in range(B)]).astype(np.float32)
    cms = torch.stack([O.render_confmaps(pts[b], S, 2, 2.5 * 2 / 2) for b in range(B)])
    cms[0, 0] = 0.05  # below threshold everywhere -> NaN
    cms[1, 1, 40:42, 90:93] = 2.0  # a plateau: first column / first row containing the maximum
    cms[2, 2, 255, 255] = 3.0  # the very last pixel
    cms[3, 3, 10, 200] = cms[3, 3, 200, 10] = 4.0  # two equal maxima: x from one, y from the other (independent arg-maxes)
    out = layer.postprocess({"SingleInstanceConfmapsHead": cms.to(DEV)}, PreprocInfo(eff_scale=torch.ones(B), output_stride=2))
    rk, rv = O.single_instance_postprocess(cms, 2)
    k = out.pred_keypoints.cpu().numpy()
    assert k.shape == tuple(rk.shape) == (B, 1, N, 2)
    assert np.array_equal(np.isnan(k), np.isnan(rk.numpy())) and np.isnan(k[0, 0, 0]).all()
    assert np.allclose(k, rk.numpy(), atol=1e-4, equal_nan=True)
    assert np.array_equal(out.pred_peak_values.cpu().numpy(), rv.numpy())
    rough, _ = O.find_global_peaks(cms, 0.2, None)
    assert tuple(rough[3, 3].tolist()) == (10.0, 10.0)  # x of the first column holding the maximum, y of the first row: a point that is no maximum at all


def _wz(z, prefix):
    return {k[len(prefix):]: torch.from_numpy(z[k]) for k in z.files if k.startswith(prefix)}


def test_crop_gather_matches_reference():
    from sleap_nn_amd.inference.ops.crops import crop_bboxes, make_centered_bboxes

    z = G.load("topdown.npz")
    im, pts, si = torch.from_numpy(z["cropkat/image"]), torch.from_numpy(z["cropkat/pts"]), torch.from_numpy(z["cropkat/si"])
    for hw in ((8, 8), (7, 11), (16, 12)):
        bb = make_centered_bboxes(pts, hw[0], hw[1])
        assert np.allclose(bb.numpy(), z[f"cropkat/{hw[0]}x{hw[1]}/bboxes"])
        assert np.array_equal(crop_bboxes(im.to(DEV), bb, si).cpu().numpy(), z[f"cropkat/{hw[0]}x{hw[1]}/u8"])
        assert np.array_equal(crop_bboxes((im.float() / 7).to(DEV), bb, si).cpu().numpy(), z[f"cropkat/{hw[0]}x{hw[1]}/f32"])
    assert crop_bboxes(im.to(DEV), torch.zeros(0, 4, 2), torch.zeros(0)).shape[0] == 0


def test_topdown_layer_reproduces_reference():
    from sleap_nn_amd.architectures.model import Model
    from sleap_nn_amd.inference.backends import HipBackend
    from sleap_nn_amd.inference.layers import CenteredInstanceLayer, CentroidLayer, PostprocessConfig, TopDownLayer

    z = G.load("topdown.npz")
    cfg = G.config(z)
    cc, ci = cfg["centroid"], cfg["centered"]
    mc = Model("unet", cc["backbone"], cc["heads"], "centroid")
    mc.load_state_dict(_wz(z, "wc/"))
    mi = Model("unet", ci["backbone"], ci["heads"], "centered_instance")
    mi.load_state_dict(_wz(z, "wi/"))
    pc = PostprocessConfig(peak_threshold=0.03, max_instances=6)
    cl = CentroidLayer(HipBackend(mc, DEV), cc["heads"]["confmaps"]["output_stride"], max_instances=6, max_stride=cc["backbone"]["max_stride"], postprocess_config=pc)
    il = CenteredInstanceLayer(HipBackend(mi, DEV), ci["heads"]["confmaps"]["output_stride"], max_stride=ci["backbone"]["max_stride"], postprocess_config=PostprocessConfig(peak_threshold=0.03))
    td = TopDownLayer(cl, il, (cfg["crop_size"], cfg["crop_size"]), return_crops=True)
    img = torch.from_numpy(z["image"])
    out = td.predict(img)
    assert np.allclose(out.pred_centroids.cpu().numpy(), z["centroids"], atol=1e-3, equal_nan=True)
    assert np.allclose(out.pred_centroid_values.cpu().numpy(), z["centroid_vals"], atol=CMS_ATOL, equal_nan=True)
    idx = z["valid_idx"]
    crops = out.crops.cpu().numpy()[idx[:, 0], idx[:, 1]]
    assert np.array_equal(crops, z["crops"])  # bit-exact uint8 crops
    ck = out.pred_crop_keypoints.cpu().numpy()[idx[:, 0], idx[:, 1]]
    assert np.allclose(ck, z["crop_peaks"], atol=1e-3, equal_nan=True)
    kimg = out.pred_keypoints.cpu().numpy()[idx[:, 0], idx[:, 1]]
    assert np.allclose(kimg, z["crop_peaks"] + z["bboxes"][:, 0][:, None, :], atol=1e-3, equal_nan=True)
    assert np.allclose(out.instance_bboxes.cpu().numpy()[idx[:, 0], idx[:, 1]], z["bboxes"], atol=1e-3)
    # the pipelined predictor (stage 1 of batch i + 1 enqueued before the counts of batch i are read) returns what predict returns, batch by batch;
    # max_instances = None sizes the outputs by the counts it reads
    from sleap_nn_amd.inference.predictor import Predictor

    frames = img.reshape(-1, *img.shape[-3:])
    frames = torch.cat([frames, frames.flip(-1), frames.flip(-2)], 0)
    # (a second copy of the layer pair: with it consecutive batches alternate between two HIP streams)
    mc2 = Model("unet", cc["backbone"], cc["heads"], "centroid")
    mc2.load_state_dict(_wz(z, "wc/"))
    mi2 = Model("unet", ci["backbone"], ci["heads"], "centered_instance")
    mi2.load_state_dict(_wz(z, "wi/"))
    td2 = TopDownLayer(CentroidLayer(HipBackend(mc2, DEV), cc["heads"]["confmaps"]["output_stride"], max_instances=6, max_stride=cc["backbone"]["max_stride"], postprocess_config=pc),
                       CenteredInstanceLayer(HipBackend(mi2, DEV), ci["heads"]["confmaps"]["output_stride"], max_stride=ci["backbone"]["max_stride"], postprocess_config=PostprocessConfig(peak_threshold=0.03)),
                       (cfg["crop_size"], cfg["crop_size"]), return_crops=True)
    for bs, reps in ((1, []), (2, []), (1, [td2]), (2, [td2])):
        outs = Predictor(td, batch_size=bs, replicas=reps).predict(frames)
        assert len(outs) == (frames.shape[0] + bs - 1) // bs
        for s0, o in zip(range(0, frames.shape[0], bs), outs):
            r = td.predict(frames[s0 : s0 + bs])
            for f in ("pred_keypoints", "pred_crop_keypoints", "pred_peak_values", "pred_centroids", "pred_centroid_values", "instance_bboxes"):
                assert np.array_equal(getattr(o, f).cpu().numpy(), getattr(r, f).cpu().numpy(), equal_nan=True), (bs, s0, f)
    cl.postprocess_config = PostprocessConfig(peak_threshold=0.03)
    cl.max_instances = None
    o_none = td.predict(img)
    n_max = int((~torch.isnan(out.pred_centroids[..., 0])).sum(1).max())
    assert o_none.pred_centroids.shape[1] == n_max and np.array_equal(o_none.pred_keypoints.cpu().numpy(), out.pred_keypoints.cpu().numpy()[:, :n_max], equal_nan=True)
    assert np.allclose(out.pred_peak_values.cpu().numpy()[idx[:, 0], idx[:, 1]], z["crop_peak_vals"], atol=CMS_ATOL)


@pytest.mark.parametrize("tag", ["up", "down"])
def test_topdown_layer_with_an_active_sizematcher_reproduces_the_reference_layer(tag):
    """the reference's TopDownLayer.predict with the centroid layer's sizematcher ACTIVE (eff_scale 1.125 / 0.9167: frames resized and padded to
    max_height x max_width) -- `topdown_sized.npz` holds what the reference layer itself returns (oracle/gen_golden.py::topdown_sized_fixture).  Stage 2 works in sized space:
    boxes around centroid * eff_scale, crops cut from the SIZED frame (bit-exact uint8), keypoints = (crop keypoints + sized top-left) / eff_scale, boxes / eff_scale
    (layers/topdown.py:127-150, 262-267).  The round-5 device path boxed the image-space centroid and cropped the raw frame: another scale than the reference's."""
    from sleap_nn_amd.architectures.model import Model
    from sleap_nn_amd.inference.backends import HipBackend
    from sleap_nn_amd.inference.layers import CenteredInstanceLayer, CentroidLayer, PostprocessConfig, PreprocessConfig, TopDownLayer

    z0, z = G.load("topdown.npz"), G.load("topdown_sized.npz")
    cfg = G.config(z0)
    cc, ci = cfg["centroid"], cfg["centered"]
    mc = Model("unet", cc["backbone"], cc["heads"], "centroid")
    mc.load_state_dict(_wz(z0, "wc/"))
    mi = Model("unet", ci["backbone"], ci["heads"], "centered_instance")
    mi.load_state_dict(_wz(z0, "wi/"))
    mh, mw = (int(v) for v in z[f"{tag}/max_hw"])
    cl = CentroidLayer(HipBackend(mc, DEV), cc["heads"]["confmaps"]["output_stride"], max_instances=6, max_stride=cc["backbone"]["max_stride"],
                       preprocess_config=PreprocessConfig(max_height=mh, max_width=mw), postprocess_config=PostprocessConfig(peak_threshold=0.03, max_instances=6))
    il = CenteredInstanceLayer(HipBackend(mi, DEV), ci["heads"]["confmaps"]["output_stride"], max_stride=ci["backbone"]["max_stride"], postprocess_config=PostprocessConfig(peak_threshold=0.03))
    td = TopDownLayer(cl, il, (cfg["crop_size"], cfg["crop_size"]), return_crops=True)
    img = torch.from_numpy(z["image"])
    for out in (td.predict(img), td._predict_with_host_nms(img.to(DEV))):  # the device path and the reference-shaped path (centroid NMS off: same result)
        assert float(out.preprocess_info.eff_scale[0]) != 1.0
        valid = ~np.isnan(z[f"{tag}/pred_centroids"][..., 0])
        assert np.array_equal(~np.isnan(out.pred_centroids.cpu().numpy()[..., 0]), valid) and valid.sum() >= 4
        assert np.allclose(out.pred_centroids.cpu().numpy(), z[f"{tag}/pred_centroids"], atol=2e-3, equal_nan=True)
        assert np.allclose(out.pred_centroid_values.cpu().numpy(), z[f"{tag}/pred_centroid_values"], atol=CMS_ATOL, equal_nan=True)
        assert np.allclose(out.instance_bboxes.cpu().numpy(), z[f"{tag}/instance_bboxes"], atol=2e-3, equal_nan=True)
        assert np.array_equal(out.crops.cpu().numpy()[valid], z[f"{tag}/crops"][valid])  # bit-exact uint8 crops of the sizematched frame
        assert np.allclose(out.pred_crop_keypoints.cpu().numpy(), z[f"{tag}/pred_crop_keypoints"], atol=1e-3, equal_nan=True)
        assert np.allclose(out.pred_keypoints.cpu().numpy(), z[f"{tag}/pred_keypoints"], atol=2e-3, equal_nan=True)
        assert np.allclose(out.pred_peak_values.cpu().numpy(), z[f"{tag}/pred_peak_values"], atol=CMS_ATOL, equal_nan=True)


def test_multiclass_bottomup_layer_reproduces_reference_golden():
    from sleap_nn_amd.architectures.model import Model
    from sleap_nn_amd.inference.backends import HipBackend
    from sleap_nn_amd.inference.layers import BottomUpMultiClassLayer, PostprocessConfig
    from sleap_nn_amd.inference.ops.identity import classify_peaks_from_maps

    z = G.load("multiclass.npz")
    cfg = G.config(z)
    m = Model("unet", cfg["backbone"], cfg["heads"], "multi_class_bottomup")
    m.load_state_dict(G.weights(z))
    h = cfg["heads"]
    layer = BottomUpMultiClassLayer(HipBackend(m, DEV), h["confmaps"]["output_stride"], h["class_maps"]["output_stride"], max_stride=cfg["backbone"]["max_stride"],
                                    postprocess_config=PostprocessConfig(peak_threshold=0.05))
    raw = layer.backend(torch.from_numpy(z["image"]))
    for k in ("MultiInstanceConfmapsHead", "ClassMapsHead"):
        assert (raw[k].cpu() - torch.from_numpy(z["out/" + k])).abs().max().item() <= CMS_ATOL  # sigmoid head included
    out = layer.predict(torch.from_numpy(z["image"]).squeeze(1))
    k = out.pred_keypoints.numpy() / cfg["preprocessing"]["scale"]  # golden captured with input scale 0.5
    assert np.array_equal(np.isnan(k), np.isnan(z["gold_peaks"]))
    assert np.allclose(k, z["gold_peaks"], atol=1e-3, equal_nan=True)
    assert np.allclose(out.pred_peak_values.numpy(), z["peak_vals"], atol=CMS_ATOL, equal_nan=True)
    # the pipelined predictor (GPU stage of batch i + 1 enqueued before the host stage of batch i is collected) returns what predict returns, batch by batch
    from sleap_nn_amd.inference.predictor import Predictor

    frames = torch.from_numpy(z["image"]).squeeze(1)
    frames = torch.cat([frames, frames.flip(-1), frames.flip(-2)], 0)
    outs = Predictor(layer, batch_size=2).predict(frames)
    assert len(outs) == (frames.shape[0] + 1) // 2
    for s0, o in zip(range(0, frames.shape[0], 2), outs):
        r = layer.predict(frames[s0 : s0 + 2])
        for f in ("pred_keypoints", "pred_peak_values", "instance_scores", "instance_tracking_scores"):
            assert np.array_equal(getattr(o, f).numpy(), getattr(r, f).numpy(), equal_nan=True), (s0, f)
    # randomized KAT (ties, .5 coordinates) straight through the ops
    p, v, c = classify_peaks_from_maps(torch.from_numpy(z["kat/class_maps"]).to(DEV), torch.from_numpy(z["kat/pts"]).to(DEV), torch.from_numpy(z["kat/vals"]).to(DEV),
                                       torch.from_numpy(z["kat/sb"]).to(DEV), torch.from_numpy(z["kat/sc"]).to(DEV), 4)
    assert np.array_equal(np.nan_to_num(p.numpy(), nan=-9), np.nan_to_num(z["kat/points"], nan=-9))
    assert np.array_equal(np.nan_to_num(c.numpy(), nan=-9), np.nan_to_num(z["kat/class_probs"], nan=-9))


def test_predictor_from_run_directory_matches_golden():
    import os

    from sleap_nn_amd.inference.predictor import Predictor

    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ckpt_dirs")
    z = G.load("ckpt_bottomup.npz")
    p = Predictor.from_model_paths([os.path.join(root, "minimal_instance_bottomup")], device=DEV, batch_size=1, peak_threshold=0.05)
    frames = torch.from_numpy(z["image"]).squeeze(1)  # (2, 1, 384, 384)
    gp = G.ragged(z, "gold_peaks")
    for pipelined in (True, False):
        outs = p.predict(frames, pipelined=pipelined)
        assert len(outs) == 2 and [int(o.frame_indices[0]) for o in outs] == [0, 1]
        for b, o in enumerate(outs):
            n = gp[b].shape[0]
            k = o.pred_keypoints.numpy()[0]
            assert k.shape[0] >= n
            assert np.allclose(k[:n], gp[b].reshape(n, -1, 2), atol=1e-3, equal_nan=True)
    zs = G.load("ckpt_single_instance.npz")
    ps = Predictor.from_model_paths([os.path.join(root, "minimal_instance_single_instance")], device=DEV, batch_size=2, peak_threshold=0.3)
    pc = ps.layer.preprocess_config
    assert (pc.max_height, pc.max_width, pc.scale) == (320, 560, 0.5)  # read from the run directory's training_config.yaml
    from sleap_nn_amd.inference.layers import PreprocessConfig

    ps.layer.preprocess_config = PreprocessConfig()  # the golden frames are the reference's ALREADY preprocessed 160x280 model inputs
    o = ps.predict(torch.from_numpy(zs["image"]).squeeze(1))[0]
    assert np.allclose(o.pred_keypoints[:, 0].cpu().numpy() / 0.5, zs["gold_peaks"], atol=1e-3, equal_nan=True)
    # the pipelined path of a device-only layer (one hipGraph launch per batch incl. the preprocessing, copies of the layer on streams of their own) against the plain loop:
    # the run directory's own preprocessing (sizematcher to 320 x 560, input scale 0.5) on 7 frames of another size, batches of 2 -- ragged last batch
    ps2 = Predictor.from_model_paths([os.path.join(root, "minimal_instance_single_instance")], device=DEV, batch_size=2, peak_threshold=0.0)
    assert len(ps2.replicas) == 2  # (from_model_paths(streams=3): three copies of a small network)
    g = torch.Generator().manual_seed(3)
    vid = torch.randint(0, 256, (7, 1, 300, 500), dtype=torch.uint8, generator=g)
    ref_outs = ps2.predict(vid, pipelined=False)
    for _ in range(2):
        got_outs = ps2.predict(vid)
        assert len(got_outs) == len(ref_outs) == 4
        for a_, b_ in zip(got_outs, ref_outs):
            assert torch.equal(a_.frame_indices, b_.frame_indices) and a_.preprocess_info.original_size == b_.preprocess_info.original_size
            assert torch.equal(a_.pred_keypoints.cpu(), b_.pred_keypoints.cpu()) and torch.equal(a_.pred_peak_values.cpu(), b_.pred_peak_values.cpu())
    assert torch.isfinite(ref_outs[0].pred_keypoints).all()


def test_fused_pool_epilogue_odd_sizes_and_unfused_equivalence():
    """Encoder-only nets (head on the middle block) accept any input size: exercises the zero-padded
    odd-size pooling of the fused conv+pool epilogue in both conv kernels, against the oracle."""
    from sleap_nn_amd import _lib as L
    from sleap_nn_amd.architectures.model import Model

    for filters, hw in ((32, (36, 44)), (64, (72, 52)), (20, (17, 33))):
        bb = {"in_channels": 1, "kernel_size": 3, "filters": filters, "filters_rate": 2, "max_stride": 8, "stem_stride": None, "middle_block": True,
              "up_interpolate": True, "stacks": 1, "convs_per_block": 2, "output_stride": 8}
        heads = {"confmaps": {"part_names": ["a", "b", "c"], "output_stride": 8}}
        sd = O.init_state(bb, heads, "single_instance", seed=filters, head_scale=1.0)
        g = torch.Generator().manual_seed(filters)
        img = torch.randint(0, 256, (2, 1, hw[0], hw[1]), dtype=torch.uint8, generator=g)
        ref = O.model_forward(sd, bb, heads, "single_instance", img)["SingleInstanceConfmapsHead"]
        m = Model("unet", bb, heads, "single_instance")
        m.load_state_dict(sd)
        assert any(o.kind == L.OP_CONV and o.dst2 >= 0 for o in m.ops) and not any(o.kind == L.OP_POOL for o in m.ops)
        out = m.to(DEV)(img.to(DEV))["SingleInstanceConfmapsHead"].cpu()
        assert out.shape == ref.shape
        assert (out - ref).abs().max().item() <= CMS_ATOL * max(1.0, ref.abs().max().item()), (filters, hw)


def test_multiclass_topdown_reproduces_reference_golden():
    """multi_class_topdown: ClassVectorsHead on the GPU (global max pool, FC stack on the row GEMM, softmax),
    per-frame Hungarian class assignment, and the full centroid -> crops -> keypoints + identity pipeline vs the
    reference's golden pickle (keypoints within 2e-3 px as for plain top-down; class indices identical)."""
    from sleap_nn_amd.architectures.model import Model
    from sleap_nn_amd.inference.backends import HipBackend
    from sleap_nn_amd.inference.layers import CenteredInstanceMultiClassLayer, CentroidLayer, PostprocessConfig, TopDownMultiClassLayer

    g = G.load("multiclass_topdown.npz")
    cfg = json.loads(str(g["config_json"]))
    sd = {k[2:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("w/")}
    m = Model("unet", cfg["backbone"], cfg["heads"], cfg["model_type"])
    m.load_state_dict(sd, strict=True)
    m.to(DEV)
    out = m(torch.from_numpy(g["crops"]).to(DEV))
    torch.cuda.synchronize()
    assert (out["CenteredInstanceConfmapsHead"].cpu() - torch.from_numpy(g["out/CenteredInstanceConfmapsHead"])).abs().max().item() <= CMS_ATOL
    cv = out["ClassVectorsHead"].cpu().numpy()
    assert cv.shape == g["out/ClassVectorsHead"].shape
    np.testing.assert_allclose(cv, g["out/ClassVectorsHead"], rtol=2e-3, atol=1e-7)  # probabilities down to 1e-20: relative bar
    # stage-2 layer on the golden's own crops: joint assignment inside the layer, per-frame in the composed layer
    pc = PostprocessConfig(peak_threshold=0.03, refinement="integral", integral_patch_size=5)
    l2 = CenteredInstanceMultiClassLayer(HipBackend(m, DEV), output_stride=cfg["heads"]["confmaps"]["output_stride"], max_stride=cfg["backbone"]["max_stride"],
                                         postprocess_config=pc, class_names=cfg["heads"]["class_vectors"]["classes"])
    o2 = l2.predict(torch.from_numpy(g["crops"]).to(DEV))
    np.testing.assert_allclose(o2.pred_keypoints.squeeze(1).cpu().numpy(), g["crop_peaks"], rtol=0, atol=2e-3, equal_nan=True)
    # composed pipeline on the full frames with the centroid fixture model of topdown.npz
    z = G.load("topdown.npz")
    tcfg = json.loads(str(z["config_json"]))
    mc = Model("unet", tcfg["centroid"]["backbone"], tcfg["centroid"]["heads"], "centroid")
    mc.load_state_dict({k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("wc/")}, strict=True)
    mc.to(DEV)
    cl = CentroidLayer(HipBackend(mc, DEV), output_stride=tcfg["centroid"]["heads"]["confmaps"]["output_stride"], max_stride=tcfg["centroid"]["backbone"]["max_stride"],
                       postprocess_config=PostprocessConfig(peak_threshold=0.03, refinement="integral", integral_patch_size=5, max_instances=6))
    td = TopDownMultiClassLayer(cl, l2, (cfg["crop_size"], cfg["crop_size"]))
    frames = torch.from_numpy(g["frames"])
    res = td.predict(frames.to(DEV)).cpu()
    fi = g["crop_frame"]
    for f in range(frames.shape[0]):
        gold_k = g["gold_pred_instance_peaks"][fi == f]
        gold_c = g["gold_pred_class_inds"][fi == f]
        gold_cent = g["gold_pred_centroids"][fi == f]
        got_cent = res.pred_centroids[f].numpy()
        live = ~np.isnan(got_cent).any(axis=1)
        assert live.sum() == len(gold_cent)
        for k_ref, c_ref, ce_ref in zip(gold_k, gold_c, gold_cent):  # instances are matched through their centroids
            d = np.abs(got_cent - ce_ref[None]).sum(axis=1)
            d[~live] = np.inf
            j = int(np.argmin(d))
            assert d[j] <= 2e-2, (f, d)
            got = res.pred_keypoints[f, j].numpy()
            assert np.array_equal(np.isnan(got), np.isnan(k_ref))  # this fixture model's maps stay below the 0.03 threshold: NaN keypoints
            np.testing.assert_allclose(got, k_ref, rtol=0, atol=2e-2, equal_nan=True)
            assert int(res.pred_class_inds[f, j, 0]) == int(c_ref)
            assert torch.isfinite(res.instance_tracking_scores[f, j])
    assert class_names_ok(td.class_names, cfg)


def class_names_ok(names, cfg):
    return list(names) == list(cfg["heads"]["class_vectors"]["classes"])


def test_graph_replay_equals_eager():
    """HipBackend(use_graph=True): the forward of a shape is captured once into a hipGraph and replayed; outputs
    must be bit-identical to the eager launches (same kernels, same order) for every replay, also after the input changes.
    (Latency is reported, not asserted: wall-clock assertions flake.)"""
    import time

    from sleap_nn_amd.inference.backends import HipBackend

    z = G.load("unet_tiny_interp.npz")
    cfg = G.config(z)
    m1, m2 = _model(cfg, G.weights(z)), _model(cfg, G.weights(z))
    eager, graph = HipBackend(m1, DEV), HipBackend(m2, DEV, use_graph=True)
    g = torch.Generator().manual_seed(2)
    for rep in range(3):
        img = torch.randint(0, 256, (1, cfg["backbone"]["in_channels"], 64, 64), dtype=torch.uint8, generator=g).to(DEV)
        a, b = eager(img), graph(img)
        torch.cuda.synchronize()
        for k in a:
            assert torch.equal(a[k], b[k]), (rep, k)
    assert len(graph._graphs) == 1
    t = {}
    for name, be in (("eager", eager), ("graph", graph)):
        for _ in range(5):
            be(img)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(50):
            be(img)
        torch.cuda.synchronize()
        t[name] = (time.perf_counter() - t0) / 50
    print(f"latency per 64x64 frame: eager {t['eager'] * 1e3:.3f} ms, graph {t['graph'] * 1e3:.3f} ms")


def test_graph_entries_survive_workspace_growth_and_weight_reload():
    """A captured graph holds raw pointers into the model's workspace and packed weights.  Capture a small shape, then a
    larger one (the workspace is reallocated), then replay the small one: it must equal eager -- stale entries are
    re-captured, never replayed into freed memory.  Same after load_state_dict (the handle is rebuilt)."""
    from sleap_nn_amd.inference.backends import HipBackend

    z = G.load("unet_tiny_interp.npz")
    cfg = G.config(z)
    w = G.weights(z)
    eager, graph = HipBackend(_model(cfg, w), DEV), HipBackend(_model(cfg, w), DEV, use_graph=True)
    g = torch.Generator().manual_seed(5)
    cin = cfg["backbone"]["in_channels"]
    small = torch.randint(0, 256, (1, cin, 64, 64), dtype=torch.uint8, generator=g).to(DEV)
    big = torch.randint(0, 256, (4, cin, 192, 256), dtype=torch.uint8, generator=g).to(DEV)

    def same(x):
        a, b = eager(x), graph(x)
        torch.cuda.synchronize()
        return all(torch.equal(a[k], b[k]) for k in a)

    assert same(small)
    gen0 = graph.model.generation
    assert same(big)
    assert graph.model.generation != gen0  # the workspace grew
    junk = torch.full((graph.model._workspace.numel() // 4,), float("nan"), device=DEV)  # whatever the allocator recycles is poisoned
    assert same(small) and same(big) and same(small)
    del junk
    w2 = {k: v * 0.5 for k, v in w.items()}
    eager.model.load_state_dict(w2)
    graph.model.load_state_dict(w2)
    assert same(small) and same(big)
    for e in graph._graphs.values():
        assert e[3] is graph.model._workspace  # every live entry pins the workspace it was captured on


def test_forward_is_bitwise_deterministic_and_stream_safe():
    """Two forwards of the same batch give bit-identical maps (fixed reduction orders, no atomics), also when the
    second one runs on a different stream and after other shapes have been through the same model handle
    (persistent workgroups, LDS rings and workspace reuse leave no state behind)."""
    z = G.load("unet_tiny_bu13.npz")
    cfg = G.config(z)
    m = _model(cfg, G.weights(z))
    g = torch.Generator().manual_seed(9)
    img = torch.randint(0, 256, (3, cfg["backbone"]["in_channels"], 96, 128), dtype=torch.uint8, generator=g).to(DEV)
    a = {k: v.clone() for k, v in m(img).items()}
    m(img[:1, :, :64, :64].contiguous())  # another shape in between
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        b = {k: v.clone() for k, v in m(img).items()}
    s.synchronize()
    torch.cuda.synchronize()
    for k in a:
        assert torch.equal(a[k], b[k]), k


@pytest.mark.parametrize("filters,max_stride,hw,out_stride", [(32, 8, (64, 64), None), (64, 8, (72, 52), None), (32, 8, (36, 44), None),
                                                             (32, 16, (128, 160), 2), (48, 8, (80, 48), 4), (64, 4, (50, 70), None)])
def test_winograd_2d_kernel_matches_oracle_and_the_other_conv_kernels(filters, max_stride, hw, out_stride):
    """conv3x3_wino2d_kernel (F(2x2,3x3), every 3x3 conv with >= 64 output and >= 32 input channels) against the oracle at the
    confmap bar, and against the F(2,3)-along-x and the direct kernels of the same handle options: tiles cut by the image border
    (sizes that are no multiple of 16), the fused pool epilogue with odd sizes, N tiles cut by Cout (48 * 2 = 96 channels), the
    two-source concat convs of a decoder, several tiles per workgroup (persistent walk) -- all three kernels agree to a few ulp
    of the tensor's scale."""
    from sleap_nn_amd.architectures.model import Model

    os_ = out_stride or max_stride
    bb = {"in_channels": 1, "kernel_size": 3, "filters": filters, "filters_rate": 2, "max_stride": max_stride, "stem_stride": None, "middle_block": True,
          "up_interpolate": True, "stacks": 1, "convs_per_block": 2, "output_stride": os_}
    heads = {"confmaps": {"part_names": ["a", "b", "c"], "output_stride": os_}}
    sd = O.init_state(bb, heads, "single_instance", seed=filters + hw[0], head_scale=1.0)
    g = torch.Generator().manual_seed(hw[1])
    img = torch.randint(0, 256, (3, 1, hw[0], hw[1]), dtype=torch.uint8, generator=g)
    ref = O.model_forward(sd, bb, heads, "single_instance", img)["SingleInstanceConfmapsHead"]
    outs = {}
    for name, opts in (("w2d", {}), ("w1d", {"conv_wino2d": 0}), ("direct", {"conv_wino2d": 0, "conv_wino": 0})):
        m = Model("unet", bb, heads, "single_instance")
        m.load_state_dict(sd)
        for k, v in opts.items():
            m.set_option(k, v)
        outs[name] = m.to(DEV)(img.to(DEV))["SingleInstanceConfmapsHead"].cpu()
        if name == "w2d":
            assert m.get_option("conv_wino2d") == 1.0  # the default
    scale = max(1.0, ref.abs().max().item())
    assert (outs["w2d"] - ref).abs().max().item() <= CMS_ATOL * scale
    for other in ("w1d", "direct"):
        assert (outs["w2d"] - outs[other]).abs().max().item() <= 2e-5 * ref.abs().max().item(), other
    again = Model("unet", bb, heads, "single_instance")
    again.load_state_dict(sd)
    assert torch.equal(again.to(DEV)(img.to(DEV))["SingleInstanceConfmapsHead"].cpu(), outs["w2d"])  # run-to-run bitwise


@pytest.mark.parametrize("wino4", [0, 3])
def test_half_empty_n_tiles_and_rotated_tile_dealing_match_oracle(wino4):
    """filters = 24, rate 2 -> 24 / 48 / 96 / 192 channels: padded channel counts of 32 and 96 have a last N tile with only its first 32 channels real.
    Both Winograd kernels skip that half's MFMAs (the F(4x4,3x3) kernel: the waves of N half 1) and, where a layer has several N tiles, rotate the N tiles
    over the persistent workgroups by round -- 24 frames of 256 x 256 give the 96-channel level (64 x 64) 384 pixel tiles x 2 N tiles = three rounds of the
    chip, so a wrong rotation (a (pixel tile, N tile) pair computed twice or never) cannot hide.  Against the oracle at the head bar and against the
    direct kernels; run-to-run bitwise."""
    from sleap_nn_amd import _lib as L
    from sleap_nn_amd.architectures.model import Model

    bb = {"in_channels": 1, "kernel_size": 3, "filters": 24, "filters_rate": 2, "max_stride": 8, "stem_stride": None, "middle_block": True,
          "up_interpolate": True, "stacks": 1, "convs_per_block": 2, "output_stride": 2}
    heads = {"confmaps": {"part_names": ["a", "b"], "output_stride": 2}}
    sd = O.init_state(bb, heads, "single_instance", seed=91, head_scale=1.0)
    g = torch.Generator().manual_seed(92)
    img = torch.randint(0, 256, (24, 1, 256, 256), dtype=torch.uint8, generator=g)
    ref = O.model_forward(sd, bb, heads, "single_instance", img[:3])["SingleInstanceConfmapsHead"]
    outs = {}
    for name, opts in (("wino", {"conv_wino4": wino4}), ("direct", {"conv_wino4": 0, "conv_wino2d": 0, "conv_wino": 0})):
        m = Model("unet", bb, heads, "single_instance")
        m.load_state_dict(sd)
        for k, v in opts.items():
            m.set_option(k, v)
        m.to(DEV)
        outs[name] = m(img.to(DEV))["SingleInstanceConfmapsHead"].cpu()
        if name == "wino":
            kinds = {L.KV_NAMES.get(c, "") for c in m.last_kernels()}
            assert any("wino2d" in k for k in kinds) and (wino4 == 0 or any("wino4" in k for k in kinds)), kinds
            assert torch.equal(m(img.to(DEV))["SingleInstanceConfmapsHead"].cpu(), outs["wino"])  # run-to-run bitwise
    scale = max(1.0, ref.abs().max().item())
    assert (outs["wino"][:3] - ref).abs().max().item() <= max(CMS_ATOL, W4_RTOL * scale)
    assert (outs["wino"] - outs["direct"]).abs().max().item() <= 3e-5 * outs["direct"].abs().max().item()  # all 24 frames: every (pixel tile, N tile) pair


# Relative bar of the F(4x4,3x3) layers (conv3x3_wino4_kernel): the transforms carry coefficients up to 8 / 5 / (1/24), so the result sits ~2-3x
# further from the fp64 convolution than F(2x2,3x3) does -- measured on these networks: heads 1.3e-6 ... 2.7e-6 of their scale (F(2x2,3x3):
# 0.8e-6 ... 1.2e-6), single activations up to 6.3e-6 -- stated here as 1e-5 of the tensor's scale, ten times inside the 1e-4 bar.
W4_RTOL = 1e-5


@pytest.mark.parametrize("filters,max_stride,hw,out_stride,batch", [(32, 8, (128, 128), None, 2), (16, 32, (128, 192), 4, 3), (32, 16, (128, 160), 2, 2),
                                                                   (64, 4, (48, 80), None, 2), (32, 8, (100, 132), None, 2), (16, 32, (256, 384), 4, 9),
                                                                   (32, 16, (128, 192), 8, 2)])  # (output stride 8: the stride-2 / -4 encoder convs' full-resolution outputs are unread -> pool-only stores)
def test_winograd_f4x4_kernel_and_folded_bilinear_match_oracle_and_the_f2x2_kernel(filters, max_stride, hw, out_stride, batch):
    """conv3x3_wino4_kernel (Winograd F(4x4,3x3): 3x3 convs with N tile 64 and >= 64 padded input channels, the encoder's fused 2x2 max pool included) with the decoder's
    bilinear x2 folded into its input transform (inference plans: the up-sampled tensor never exists), against the oracle and the
    F(2x2,3x3) kernel: two-source concat convs at three decoder levels (tiles at every image border: zero padding of the up-sampled
    tensor vs the clamped low-resolution indices), one-source middle / refine convs, maps that cut the 32 x 16 workgroup tile,
    several tiles per persistent workgroup (the 9-frame case), and a map size that is no multiple of 4 (-> the F(2x2,3x3) kernel keeps
    the layer, the separate bilinear kernel runs).  `conv_wino4 = 2` runs the kernel WITHOUT the fold on a plan that keeps every
    activation, so each layer's output is compared on its own."""
    from sleap_nn_amd import _lib as L
    from sleap_nn_amd.architectures.model import Model

    os_ = out_stride or max_stride
    bb = {"in_channels": 1, "kernel_size": 3, "filters": filters, "filters_rate": 2, "max_stride": max_stride, "stem_stride": None, "middle_block": True,
          "up_interpolate": True, "stacks": 1, "convs_per_block": 2, "output_stride": os_}
    heads = {"confmaps": {"part_names": ["a", "b", "c"], "output_stride": os_}}
    sd = O.init_state(bb, heads, "single_instance", seed=filters + hw[0], head_scale=1.0)
    g = torch.Generator().manual_seed(hw[1])
    img = torch.randint(0, 256, (batch, 1, hw[0], hw[1]), dtype=torch.uint8, generator=g)
    collect = {}
    ref = O.model_forward(sd, bb, heads, "single_instance", img, collect=collect)["SingleInstanceConfmapsHead"]
    scale = ref.abs().max().item()
    outs, n4 = {}, {}
    # (conv_wino4 = 3 forces the kernel wherever the shape fits: at these sizes the default's cost estimate -- rounds of the chip -- keeps F(2x2,3x3))
    for name, opts, keep in (("default", {}, False), ("fold", {"conv_wino4": 3, "conv_smallmap": 0}, False), ("nofold", {"conv_wino4": 3, "upsample_fold": 0, "conv_smallmap": 0}, False), ("every_plan", {"conv_wino4": 3, "conv_smallmap": 0}, True), ("f2x2", {"conv_wino4": 0, "conv_smallmap": 0}, False)):  # (conv_smallmap = 0: this test is about the F(4x4,3x3) kernel; the small-map kernel would take these layers from it at these batch sizes)
        m = Model("unet", bb, heads, "single_instance")
        m.load_state_dict(sd)
        for k, v in opts.items():
            m.set_option(k, v)
        m.to(DEV).set_keep_activations(keep)
        outs[name] = m(img.to(DEV))["SingleInstanceConfmapsHead"].cpu()
        kv = m.last_kernels()
        n4[name] = sum(1 for c in kv if c == L.KV_WINO4)
        if name == "default":
            assert m.get_option("conv_wino4") == 1.0 and m.get_option("upsample_fold") == 1.0
        if name == "fold":
            ups = [i for i, op in enumerate(m.ops) if op.kind == L.OP_UPSAMPLE]
            folded = [i for i in ups if kv[i + 1] == L.KV_WINO4]
            pooled4 = sum(1 for r, c in zip(m.op_table(batch, hw[0], hw[1]), kv) if "+pool" in r["label"] and c == L.KV_WINO4)  # encoder convs whose 2x2 max pool rides in the kernel's output stage
        if keep:
            checked = 0
            for lab, t in collect.items():
                if lab not in m.backbone.labels:
                    continue
                try:
                    got = m.read_activation(lab, t.shape[0], t.shape[-2:]).cpu()
                except KeyError:
                    continue  # fused away (stem)
                assert (got - t).abs().max().item() <= W4_RTOL * max(t.abs().max().item(), 1e-30), lab
                checked += 1
            assert checked >= 6
    whole_tiles = all((hw[0] // s) % 4 == 0 and (hw[1] // s) % 4 == 0 for s in (max_stride, max_stride // 2)) or max_stride == os_
    if hw[0] % (4 * max_stride) == 0 and hw[1] % (4 * max_stride) == 0:
        assert n4["fold"] >= 2 and n4["f2x2"] == 0 and n4["every_plan"] >= n4["nofold"] >= 2, n4
        if os_ < max_stride:
            assert folded, "a decoder's bilinear x2 must ride in the F(4x4,3x3) kernel"
        if filters >= 32:
            assert pooled4 >= 1, "an encoder conv + pool with >= 64 input channels must run on the F(4x4,3x3) kernel (fused pool)"
    for name in ("default", "fold", "nofold", "every_plan", "f2x2"):
        assert (outs[name] - ref).abs().max().item() <= W4_RTOL * scale, (name, n4)
    assert (outs["fold"] - outs["f2x2"]).abs().max().item() <= W4_RTOL * scale
    again = Model("unet", bb, heads, "single_instance")
    again.load_state_dict(sd)
    again.set_option("conv_wino4", 3).set_option("conv_smallmap", 0)
    assert torch.equal(again.to(DEV)(img.to(DEV))["SingleInstanceConfmapsHead"].cpu(), outs["fold"])  # run-to-run bitwise


@pytest.mark.parametrize("hw,max_stride", [((64, 64), 8), ((36, 44), 8), ((17, 33), 4), ((96, 80), 4), ((130, 70), 4)])
def test_wave_private_winograd_kernel_matches_oracle_and_the_1d_kernel(hw, max_stride):
    """conv3x3_w16_kernel (Cout 32, Cin 16 / 32: the second encoder block of a filters = 16 UNet -- 16 -> 32 and 32 -> 32 + fused pool)
    on sizes that cut its 16x32-pixel workgroup tiles and its waves' 16x4 strips, with odd sizes through the zero-padded pool,
    against the oracle and against the F(2,3) kernel the same layers run with ``conv_w16 = 0``."""
    from sleap_nn_amd.architectures.model import Model

    bb = {"in_channels": 1, "kernel_size": 3, "filters": 16, "filters_rate": 2, "max_stride": max_stride, "stem_stride": None, "middle_block": True,
          "up_interpolate": True, "stacks": 1, "convs_per_block": 2, "output_stride": max_stride}
    heads = {"confmaps": {"part_names": ["a", "b", "c"], "output_stride": max_stride}}
    sd = O.init_state(bb, heads, "single_instance", seed=hw[0], head_scale=1.0)
    g = torch.Generator().manual_seed(hw[1])
    img = torch.randint(0, 256, (3, 1, hw[0], hw[1]), dtype=torch.uint8, generator=g)
    ref = O.model_forward(sd, bb, heads, "single_instance", img)["SingleInstanceConfmapsHead"]
    outs = {}
    for name, v in (("w16", 1), ("w1d", 0)):
        m = Model("unet", bb, heads, "single_instance")
        m.load_state_dict(sd)
        m.set_option("conv_w16", v)
        outs[name] = m.to(DEV)(img.to(DEV))["SingleInstanceConfmapsHead"].cpu()
    assert (outs["w16"] - ref).abs().max().item() <= CMS_ATOL * max(1.0, ref.abs().max().item())
    assert (outs["w16"] - outs["w1d"]).abs().max().item() <= 2e-5 * ref.abs().max().item()


@pytest.mark.parametrize("name", ["unet_tiny_interp.npz", "unet_tiny_bu13.npz", "ckpt_bottomup.npz"])
def test_direct_convolution_kernels_still_match_golden(name):
    """The Winograd kernels are the default; the direct 9-tap kernels stay in the library (transposed convs, A/B runs)
    and are selected per handle with ``set_option`` -- the library has no process-global switches."""
    z = G.load(name)
    cfg = G.config(z)
    m = _model(cfg, G.weights(z)).set_option("conv_wino", 0).set_option("stem_wino", 0)
    out = m(torch.from_numpy(z["image"]).squeeze(1).to(DEV))
    assert m.get_option("conv_wino") == 0.0
    for k in out:
        assert np.allclose(out[k].cpu().numpy(), z["out/" + k], atol=CMS_ATOL), k
    with pytest.raises(Exception, match="unknown option"):
        m.set_option("no_such_option", 1)


def test_resize_kernel_matches_the_cpu_operator():
    """ph_resize_bilinear_aa vs the oracle restatement (itself pinned bit-exactly against torch's uint8 operator on the CPU):
    uint8 bit-exact, float32 to fp32 rounding; up- and down-scaling, one-axis and identity cases, sizematcher + input scale."""
    from sleap_nn_amd.data.resizing import apply_sizematcher, resize_bilinear_aa, resize_image

    rng = np.random.default_rng(5)
    for t in range(24):
        C, H, W = int(rng.choice([1, 3])), int(rng.integers(5, 120)), int(rng.integers(5, 120))
        oh, ow = int(rng.integers(3, 160)), int(rng.integers(3, 160))
        if t % 5 == 0:
            oh = H
        if t % 7 == 0:
            ow = W
        x = torch.from_numpy(rng.integers(0, 256, (2, C, H, W), dtype=np.uint8))
        ref = O.resize_bilinear_aa(x, (oh, ow))
        got = resize_bilinear_aa(x.to(DEV), (oh, ow)).cpu()
        assert torch.equal(got, ref), (t, C, H, W, oh, ow, int((got != ref).sum()))
        xf = torch.from_numpy(rng.random((1, C, H, W), dtype=np.float32) * 255)
        reff = O.resize_bilinear_aa(xf, (oh, ow))
        gotf = resize_bilinear_aa(xf.to(DEV), (oh, ow)).cpu()
        assert (gotf - reff).abs().max().item() <= 2e-4, (t, float((gotf - reff).abs().max()))
    frame = torch.from_numpy(rng.integers(0, 256, (3, 200, 310), dtype=np.uint8))
    for mh, mw in ((160, 160), (256, 512), (200, 310), (400, None)):
        r0, e0 = O.apply_sizematcher(frame, mh, mw)
        r1, e1 = apply_sizematcher(frame.to(DEV), mh, mw)
        assert e0 == e1 and torch.equal(r1.cpu(), r0), (mh, mw)
    assert torch.equal(resize_image(frame[None].to(DEV), 0.5).cpu(), O.resize_image(frame[None], 0.5))


def test_layer_preprocess_with_sizematcher_and_input_scale():
    """SingleInstanceLayer with max_height / max_width / scale: frames of another size go through sizematcher + input scale +
    stride padding on the GPU, and the keypoints come back in ORIGINAL frame coordinates -- against the oracle's chain."""
    from sleap_nn_amd.architectures.model import Model
    from sleap_nn_amd.inference.backends import HipBackend
    from sleap_nn_amd.inference.layers import PostprocessConfig, PreprocessConfig, SingleInstanceLayer

    bb = {"in_channels": 1, "kernel_size": 3, "filters": 8, "filters_rate": 2, "max_stride": 16, "stem_stride": None, "middle_block": True, "up_interpolate": True,
          "stacks": 1, "convs_per_block": 2, "output_stride": 2}
    heads = {"confmaps": {"part_names": ["a", "b", "c", "d"], "output_stride": 2}}
    sd = O.init_state(bb, heads, "single_instance", seed=21, head_scale=1.0)
    g = torch.Generator().manual_seed(21)
    img = torch.randint(0, 256, (2, 1, 150, 230), dtype=torch.uint8, generator=g)
    m = Model("unet", bb, heads, "single_instance")
    m.load_state_dict(sd)
    pre = PreprocessConfig(max_height=128, max_width=192, scale=0.75)
    x_ref, eff, _ = O.full_preprocess(img, 128, 192, 0.75, 16)
    cms = O.model_forward(sd, bb, heads, "single_instance", x_ref)["SingleInstanceConfmapsHead"]
    thr = float(cms.mean())
    layer = SingleInstanceLayer(HipBackend(m, DEV), 2, max_stride=16, preprocess_config=pre, postprocess_config=PostprocessConfig(peak_threshold=thr))
    x, info = layer.preprocess(img)
    assert torch.equal(x.squeeze(1).cpu(), x_ref) and torch.allclose(info.eff_scale, eff)
    out = layer.predict(img)
    rk, rv = O.single_instance_postprocess(cms, 2, peak_threshold=thr, input_scale=0.75, eff_scale=eff)
    assert np.allclose(out.pred_keypoints.cpu().numpy().reshape(rk.shape), rk.numpy(), atol=2e-3, equal_nan=True)


def test_workspace_reuse_shrinks_the_footprint_and_changes_no_bit():
    """Inference programs recycle activation slots after their last reader (handle option workspace_reuse, on by default in eval):
    the workspace of the cfg3 network shrinks by more than half, every head output is bit-identical to the one-range-per-slot plan
    (bilinear and transposed-conv decoders, all three precisions), and reading a slot back is refused while slots are shared."""
    import ctypes as C

    import bench
    from sleap_nn_amd import _lib as L
    from sleap_nn_amd.architectures.model import Model

    for name in ("unet_tiny_bu13.npz", "unet_tiny_trans.npz", "ckpt_bottomup.npz"):
        z = G.load(name)
        cfg = G.config(z)
        img = torch.from_numpy(z["image"]).squeeze(1).to(DEV)
        for prec in ("exact", "split", "fp16"):
            # (split K and the Cout-32 route are inference-plan choices with their own rounding, like conv_wino4 = 1: pinned off so that the two plans run the same kernels)
            pin = lambda mm: mm.set_option("conv_splitk", 0).set_option("conv_n32_wino2d", 0)
            a = {k: v.clone() for k, v in pin(_model(cfg, G.weights(z))).set_precision(prec).set_keep_activations(True)(img).items()}
            m = pin(_model(cfg, G.weights(z))).set_precision(prec)
            b = m(img)
            assert m.get_option("workspace_reuse") == 1.0
            for k in a:
                assert torch.equal(a[k], b[k]), (name, prec, k)
    with pytest.raises(RuntimeError, match="recycled"):
        m.read_activation(next(iter(m.backbone.labels)), 1, (8, 8))
    big = Model("unet", bench.CFG3_BB, bench.CFG3_HEADS, "bottomup").init_xavier_(seed=1).to(DEV)
    big(torch.zeros((1, 1, 64, 64), dtype=torch.uint8, device=DEV))
    shared = L.check(L.lib().ph_model_workspace_bytes(big._handle, 32, 1024, 1024))
    big.set_keep_activations(True)
    full = L.check(L.lib().ph_model_workspace_bytes(big._handle, 32, 1024, 1024))
    print(f"cfg3 x 32 frames workspace: {full / 2**30:.2f} GiB one range per slot, {shared / 2**30:.2f} GiB shared")
    assert shared < 0.5 * full


def test_unfused_program_with_shared_slots_survives_forwarded_writes():
    """run-time fusions write the NEXT op's dst one op early (pool_peephole: a conv's epilogue writes the pool that
    follows; fuse_gelu_fwd; dw_ln_fuse), so with workspace_reuse the plan must not give that dst a range the writing op is still
    reading.  The Python Model never builds that combination (eval fuses the pools into the program, train keeps every slot); a C-API
    user can: UNFUSED inference programs with workspace_reuse = 1 must give the bits of the one-range-per-slot plan."""
    import bench
    from sleap_nn_amd.architectures.model import Model

    g = torch.Generator().manual_seed(5)
    cases = [("unet", bench.CFG3_BB, bench.CFG3_HEADS, "bottomup", (2, 1, 256, 320)), ("convnext", bench.CFG4_BB, bench.CFG4_HEADS, "centered_instance", (2, 1, 96, 128))]
    for backbone, bb, heads, mt, shape in cases:
        img = torch.randint(0, 256, shape, dtype=torch.uint8, generator=g).to(DEV)
        outs = []
        # (reuse, dw_ln_fuse): the LayerNorm-in-the-depthwise-kernel fusion only exists on shared-slot plans and has its own summation
        # order, so the bitwise comparison runs with it off and a third run with it on is held to 1e-5 of the head's scale
        for reuse, ln in ((0, 0), (1, 0), (1, 1)):
            m = Model(backbone, bb, heads, mt).init_xavier_(seed=3, head_scale=1.0).to(DEV)
            m.set_fusion(False)  # the op-by-op program: conv -> pool pairs, Linear -> GELU pairs stay separate ops
            m.set_option("workspace_reuse", reuse)
            m.set_option("pool_peephole", 1)
            m.set_option("dw_ln_fuse", ln)
            m.set_option("conv_wino4", 0)  # (the F(4x4,3x3) kernel is another plan-dependent choice with its own rounding: out of this comparison)
            m.set_option("conv_splitk", 0)  # (so are split K and the Cout-32 route)
            m.set_option("conv_n32_wino2d", 0)
            outs.append({k: v.clone() for k, v in m(img).items()})
            assert m.get_option("workspace_reuse") == float(reuse)
        for k in outs[0]:
            assert torch.isfinite(outs[0][k]).all() and torch.equal(outs[0][k], outs[1][k]), (backbone, k)
            assert (outs[2][k] - outs[0][k]).abs().max().item() <= 1e-5 * outs[0][k].abs().max().item(), (backbone, k)


def test_head_fused_into_the_conv_epilogue_matches_the_head_kernel_and_the_oracle():
    """`head_fuse`: a 1x1 head that reads a 64-channel conv output is computed by that conv's F(2x2,3x3) epilogue (an MFMA on the
    accumulator registers; the tensor itself is not stored when nothing else reads it).  Same outputs as the stand-alone head kernel
    (different summation order: 1e-6 of the scale) and within the forward bar of the oracle: bottom-up (confidence maps fused, PAFs on a
    128-channel tensor not), multi-class bottom-up with BOTH heads on the same 64-channel tensor (the first fused, the sigmoid-free
    tensor still stored for the second), a sigmoid head, odd batch, and frame widths that cut tiles / break the 8-byte pixel-pair store."""
    from sleap_nn_amd import _lib as L
    from sleap_nn_amd.architectures.model import Model

    bb = {"in_channels": 1, "kernel_size": 3, "filters": 16, "filters_rate": 2, "max_stride": 16, "stem_stride": None, "middle_block": True,
          "up_interpolate": True, "stacks": 1, "convs_per_block": 2, "output_stride": 4}
    names = ["a", "b", "c", "d", "e"]
    cases = [
        ("bottomup", {"confmaps": {"part_names": names, "output_stride": 4}, "pafs": {"edges": [[names[i], names[i + 1]] for i in range(4)], "output_stride": 8}}, (96, 160), 3),
        ("multi_class_bottomup", {"confmaps": {"part_names": names, "output_stride": 4}, "class_maps": {"classes": ["x", "y", "z"], "output_stride": 4}}, (80, 112), 2),
        ("multi_class_bottomup*", {"confmaps": {"part_names": names, "output_stride": 2}, "class_maps": {"classes": ["x", "y", "z"], "output_stride": 4}}, (64, 96), 2),  # the SIGMOID head is the fused one
        ("single_instance", {"confmaps": {"part_names": names[:3], "output_stride": 4}}, (48, 176), 1),
        ("centroid", {"confmaps": {"anchor_part": None, "output_stride": 4}}, (64, 80), 2),
    ]
    for mt, heads, hw, B in cases:
        bb = dict(bb, output_stride=2 if mt.endswith("*") else 4)
        mt = mt.rstrip("*")
        sd = O.init_state(bb, heads, mt, seed=hw[1], head_scale=1.0)
        g = torch.Generator().manual_seed(hw[0])
        for k in sd:
            if k.endswith(".bias"):
                sd[k] = (torch.rand(sd[k].shape, generator=g) - 0.5) * 0.2
        img = torch.randint(0, 256, (B, 1, hw[0], hw[1]), dtype=torch.uint8, generator=g)
        ref = O.model_forward(sd, bb, heads, mt, img)
        outs = {}
        for fuse in (1, 0):
            m = Model("unet", bb, heads, mt)
            m.load_state_dict(sd)
            m.set_option("head_fuse", fuse)
            assert any(o.kind == L.OP_HEAD and o.cin0 == 64 for o in m.ops)  # a head on the 64-channel stride-4 tensor
            if heads.get("class_maps", {}).get("output_stride") == 4 and heads["confmaps"]["output_stride"] == 2:
                assert any(o.kind == L.OP_HEAD and o.cin0 == 64 and (o.flags & L.FLAG_SIGMOID) for o in m.ops)
            outs[fuse] = {k: v.cpu() for k, v in m.to(DEV)(img.to(DEV)).items()}
        for k, v in ref.items():
            scale = max(1.0, v.abs().max().item())
            assert (outs[1][k] - outs[0][k]).abs().max().item() <= 2e-6 * scale, (mt, k)
            assert (outs[1][k] - v).abs().max().item() <= CMS_ATOL * scale, (mt, k)
