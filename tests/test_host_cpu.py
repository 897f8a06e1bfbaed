"""CPU-side checks of the product: C-ABI surface, host (C++) assignment + assembly, host logic.
No GPU compute is called here."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch
from scipy.optimize import linear_sum_assignment as scipy_lsa

from oracle import cpu_ref as O
from sleap_nn_amd import _lib as L
from sleap_nn_amd.inference.ops import paf as P
from tests import _golden as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_every_declared_symbol():
    hdr = open(os.path.join(ROOT, "include", "posehip.h")).read()
    declared = set(re.findall(r"\b(ph_[a-z_0-9]+)\s*\(", hdr))
    declared -= {"ph_op_desc", "ph_model"}
    assert len(declared) >= 14
    lib = ctypes.CDLL(L.LIB_PATH)
    for name in sorted(declared):
        assert hasattr(lib, name), f"{name} declared in posehip.h but not exported"
    assert set(L.SIGNATURES) == declared
    assert L.lib().ph_version() == int(re.search(r"^#define\s+PH_VERSION\s+(\d+)", hdr, re.M).group(1))


def test_graft_entry_build_runs_and_checks_the_declared_abi_version():
    """The driver's build entry point must not raise on a tree whose library matches its header (round 3 shipped a stale literal)."""
    import __graft_entry__ as g

    g.build()
    src = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert "PH_VERSION" in src and not re.search(r"ph_version\(\)\s*==\s*\d", src)


def test_integration_binding_struct_matches_the_library():
    """The reference-side binding printed in INTEGRATION.md is executed as written: its OpDesc must have the size of the
    library's ``struct ph_op_desc`` (a 12-field struct handed to ph_model_create would mis-stride the op array), the same
    field order as the header, and the product's own binding must agree with both."""
    import ctypes as C  # noqa: F401 (used by the exec'd snippet)

    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    m = re.search(r"# <binding:OpDesc>.*?\n(.*?)# </binding:OpDesc>", doc, re.S)
    assert m, "INTEGRATION.md lost its OpDesc binding block"
    ns = {"C": ctypes}
    exec(m.group(1), ns)
    doc_desc = ns["OpDesc"]
    lib = L.lib()
    assert ctypes.sizeof(doc_desc) == lib.ph_op_desc_size() == ctypes.sizeof(L.OpDesc) == 64
    hdr = open(os.path.join(ROOT, "include", "posehip.h")).read()
    body = re.search(r"typedef struct ph_op_desc \{(.*?)\} ph_op_desc;", hdr, re.S).group(1)
    header_fields = re.findall(r"int32_t\s+(\w+);", body)
    assert [f for f, _ in doc_desc._fields_] == header_fields == [f for f, _ in L.OpDesc._fields_]


def test_hip_backend_satisfies_the_reference_protocol():
    """The reference's own runtime-checkable ``ModelBackend`` (inference/layers/backends/base.py:18-79, enforced by isinstance at
    layers/base.py:56-59) -- its members and warmup's parameters as tests/golden/backend_protocol.npz records them
    (oracle/gen_golden.py::backend_protocol_fixture) -- accepts a HipBackend-shaped object and rejects a bare object; the
    product's restated Protocol has the same members."""
    import inspect

    from sleap_nn_amd.inference.backends import HipBackend, ModelBackend

    z = G.load("backend_protocol.npz")
    ref_members, ref_warmup = {str(m) for m in z["members"]}, [str(p) for p in z["warmup_params"]]
    assert bool(z["runtime_checkable"])  # the reference's isinstance check looks for exactly these members

    def satisfies(obj):
        return all(hasattr(obj, m) for m in ref_members)

    hb = HipBackend.__new__(HipBackend)  # no GPU here: the protocol check looks at members, not state
    hb._device = torch.device("cuda", 0)
    assert satisfies(hb) and isinstance(hb, ModelBackend)
    assert not satisfies(object()) and not isinstance(object(), ModelBackend)
    members = lambda p: {n for n, _ in inspect.getmembers(p) if not n.startswith("_") or n == "__call__"}  # noqa: E731
    assert ref_members == members(ModelBackend) == {"device", "does_baked_postproc", "warmup", "__call__"}
    assert hb.device == "cuda:0" and hb.does_baked_postproc is False
    assert ref_warmup == list(inspect.signature(HipBackend.warmup).parameters) == ["self", "input_shape"]


def test_library_has_no_environment_knobs():
    """no hidden global state.  No source of the library reads the environment."""
    csrc = os.path.join(ROOT, "sleap_nn_amd", "csrc")
    for f in sorted(os.listdir(csrc)):
        assert "getenv" not in open(os.path.join(csrc, f)).read(), f


def test_unet_without_middle_block_follows_the_reference_contract():
    """unet.py:196-205: the decoder input is declared as filters * rate**down_blocks with or without the middle block, so
    middle_block=False only runs with filters_rate=1 (the reference fails on the channel mismatch at forward time)."""
    from sleap_nn_amd.architectures.unet import UNet

    base = {"in_channels": 1, "kernel_size": 3, "filters": 8, "max_stride": 8, "output_stride": 2, "convs_per_block": 2,
            "up_interpolate": True, "stacks": 1, "stem_stride": None, "middle_block": False}
    ok = UNet.from_config({**base, "filters_rate": 1})
    assert ok.max_channels == 8 and ok.decoder_stride_to_filters[8] == 8
    assert not any("middle" in k for k in ok.param_shapes)
    with pytest.raises(ValueError, match="middle_block=False"):
        UNet.from_config({**base, "filters_rate": 2})


def test_unet_wiring_equals_the_reference_over_the_whole_config_grid():
    """unet_config_grid.json.gz: convs_per_block 1/2/3 x middle_block x up_interpolate x stem_stride None/2 x filters_rate 1/1.5/2 x
    kernel_size 3/5 x in_channels 1/3 (filters 8, max_stride 8, output_stride 2, one single-instance head, a 32x48 frame), each point
    walked through the reference Model by oracle/gen_golden.py.  Where the reference builds and runs, product and oracle must have its
    backbone parameter names and shapes exactly -- the reference forwards convs_per_block to its stem, encoder and middle block but not
    to its Decoder (unet.py:203-216), whose blocks always hold two refine convs.  Where the reference fails (building: one conv per block
    with a middle block; in forward: no middle block at rate != 1), the product refuses at construction and the oracle fails as well.
    Every point is walked; the counts are the reference's own and guard against a fixture that silently shrinks."""
    import gzip
    import os

    from sleap_nn_amd.architectures.unet import UNet

    with gzip.open(os.path.join(G.GOLDEN_DIR, "unet_config_grid.json.gz"), "rt") as f:
        doc = json.load(f)
    points, heads, mt = doc["points"], doc["heads"], doc["model_type"]
    count = {s: sum(p["status"] == s for p in points) for s in ("ok", "build_raises", "forward_raises")}
    assert len(points) == 288 and count == {"ok": 144, "build_raises": 48, "forward_raises": 96}, (len(points), count)
    assert len({json.dumps(p["config"], sort_keys=True) for p in points}) == 288  # 288 different configs
    assert {p["config"]["convs_per_block"] for p in points if p["status"] == "ok"} == {1, 2, 3}
    walked = 0
    for p in points:
        bb = p["config"]
        if p["status"] == "ok":
            want = {n: tuple(shape) for n, shape in p["backbone_state"]}
            assert len(want) == len(p["backbone_state"])
            got = {k: tuple(v) for k, v in UNet.from_config(bb).param_shapes.items()}
            assert got == want, (bb, sorted(set(got) ^ set(want)))
            sd = O.init_state(bb, heads, mt)
            ora = {k: tuple(v.shape) for k, v in sd.items() if k.startswith("backbone.")}
            assert ora == want, (bb, sorted(set(ora) ^ set(want)))
            plan = O.unet_plan(bb)
            named = [n for blk in plan["stem"] + plan["enc"] + plan["dec"] for n, _, _ in blk["convs"]] + [n for convs in plan["mid"] for n, _, _ in convs]
            named += [blk["trans"][0] for blk in plan["dec"] if not blk["interp"]]
            assert sorted(named) == sorted({n.rsplit(".", 1)[0] for n in want}), bb
        else:
            with pytest.raises(ValueError):
                UNet.from_config(bb)
            with pytest.raises((AssertionError, RuntimeError, ValueError, KeyError)):
                sd = O.init_state(bb, heads, mt)
                O.model_forward(sd, bb, heads, mt, torch.zeros((1, bb["in_channels"], 32, 48), dtype=torch.uint8))
        walked += 1
    assert walked == 288
    print(f"unet config grid: {walked} points walked, 0 skipped")


def test_unet_with_stem_block_and_wide_kernels_follows_the_reference_structure():
    """stem_stride 2 (StemBlock, encoder_decoder.py:144-225): 7x7 stem convs, reference parameter names and shapes (taken from the
    golden the reference Model produced), the deepest feature at 2 x max_stride, the stem output as the last skip; kernel_size 5;
    stem_stride 4 is refused like the reference's forward refuses it."""
    from sleap_nn_amd.architectures.model import Model
    from sleap_nn_amd.architectures.unet import UNet

    for name in ("unet_tiny_stem.npz", "unet_tiny_k5.npz"):
        z = G.load(name)
        cfg = G.config(z)
        m = Model("unet", cfg["backbone"], cfg["heads"], cfg["model_type"])
        want = {k[2:]: tuple(z[k].shape) for k in z.files if k.startswith("w/")}
        assert {k: tuple(v) for k, v in m.param_shapes.items()} == want
        m.load_state_dict(G.weights(z), strict=True)
    stem = UNet.from_config(G.config(G.load("unet_tiny_stem.npz"))["backbone"])
    assert sorted(stem.decoder_stride_to_filters) == [2, 4, 8, 16] and stem.decoder_stride_to_filters[16] == 27 and stem.max_channels == 27
    assert sum(1 for o in stem.ops if o.ksize == 7 and o.kind in (L.OP_CONV, L.OP_INPUT_CONV)) == 2
    with pytest.raises(ValueError, match="stem_stride"):
        UNet.from_config({"in_channels": 1, "kernel_size": 3, "filters": 8, "filters_rate": 1.5, "max_stride": 16, "stem_stride": 4, "output_stride": 4})


def test_evaluation_metrics_match_reference():
    """evaluation.npz: the reference's compute_oks (both normalisations), its greedy instance matching and the Evaluator's
    VOC / OKS / distance / PCK metrics on 12 random frames (missing points, a far-off prediction, fewer / more predictions than
    ground truth); then the epoch-end hook on the same data handed over batch-wise in preprocessed coordinates."""
    from sleap_nn_amd.evaluation import EpochEndEvaluator, Evaluator, compute_oks
    from sleap_nn_amd.inference.outputs import Outputs

    z = G.load("evaluation.npz")
    n = int(z["n_frames"])
    gts, prs, scs = [z[f"f{f}/gt"] for f in range(n)], [z[f"f{f}/pr"] for f in range(n)], [z[f"f{f}/scores"] for f in range(n)]
    for f in range(n):
        assert np.allclose(compute_oks(gts[f], prs[f]), z[f"f{f}/oks"], rtol=1e-6, atol=1e-12)
        assert np.allclose(compute_oks(gts[f], prs[f], use_cocoeval=False, stddev=0.05, scale=900.0), z[f"f{f}/oks_paper"], rtol=1e-6, atol=1e-12)
    E = Evaluator(gts, prs, scs)
    assert np.allclose(E.pair_oks, z["pair_oks"], rtol=1e-6) and E.n_false_negatives == int(z["n_false_negatives"])
    assert np.allclose(E.dists, z["dists"], rtol=1e-6, equal_nan=True)
    m = E.evaluate()
    for k in ("oks_voc.AP", "oks_voc.AR", "oks_voc.mAP", "oks_voc.mAR", "oks_voc.precisions", "oks_voc.match_scores"):
        assert np.allclose(m["voc_metrics"][k], z["voc/" + k], rtol=1e-6), k
    assert abs(m["mOKS"]["mOKS"] - float(z["mOKS"])) < 1e-7
    assert np.allclose([m["distance_metrics"][k] for k in ("avg", "p50", "p75", "p90", "p95", "p99")], z["dist/summary"], rtol=1e-6)
    assert np.allclose([m["pck_metrics"][k] for k in ("mPCK", "PCK@5", "PCK@10")], z["pck/summary"], rtol=1e-6)
    assert np.allclose(m["pck_metrics"]["mPCK_parts"], z["pck/mPCK_parts"], rtol=1e-6)
    # epoch-end hook: batches of 4 frames, NaN-padded to a common instance count, ground truth in preprocessed space (x eff_scale)
    hook, hook1 = EpochEndEvaluator(eval_frequency=2), EpochEndEvaluator(eval_frequency=1)
    N = gts[0].shape[1]
    for lo in range(0, n, 4):
        idx = list(range(lo, min(lo + 4, n)))
        mi = max(max(len(prs[f]) for f in idx), max(len(gts[f]) for f in idx))
        kp = np.full((len(idx), mi, N, 2), np.nan, np.float32)
        vals = np.full((len(idx), mi, N), np.nan, np.float32)
        gt = np.full((len(idx), 1, mi, N, 2), np.nan, np.float32)
        eff = np.array([0.5, 1.0, 2.0, 0.75][: len(idx)], np.float32)
        for j, f in enumerate(idx):
            kp[j, : len(prs[f])] = prs[f]
            vals[j, : len(prs[f])] = scs[f][:, None]  # every node carries the instance score: its nan-mean is that score again
            gt[j, 0, : len(gts[f])] = gts[f] * eff[j]
        for h in (hook, hook1):
            h.add_batch(Outputs(pred_keypoints=torch.from_numpy(kp), pred_peak_values=torch.from_numpy(vals)), gt, eff, [len(gts[f]) for f in idx])
    assert hook.compute(epoch=0) is None  # eval_frequency 2: epoch 0 is skipped and the lists are cleared
    assert hook.compute(epoch=1) is None and not hook._pred
    m1 = hook1.compute(epoch=0)
    assert abs(m1["mOKS"]["mOKS"] - float(z["mOKS"])) < 1e-5 and abs(m1["voc_metrics"]["oks_voc.mAP"] - float(z["voc/oks_voc.mAP"])) < 1e-6
    assert np.allclose([m1["pck_metrics"][k] for k in ("mPCK", "PCK@5", "PCK@10")], z["pck/summary"], atol=1e-6)


def test_product_does_not_import_oracle():
    for dp, _, files in os.walk(os.path.join(ROOT, "sleap_nn_amd")):
        for f in files:
            if f.endswith(".py"):
                src = open(os.path.join(dp, f)).read()
                assert "oracle" not in src.replace("# oracle", ""), f"{f} references the oracle"


def _same_assignment(cost):
    r0, c0 = scipy_lsa(cost)
    r1, c1 = P.linear_sum_assignment(cost)
    assert np.array_equal(r0, r1) and np.array_equal(c0, c1), (cost, r0, c0, r1, c1)


def test_lsap_matches_scipy_including_ties():
    rng = np.random.RandomState(0)
    n = 0
    for trial in range(4000):
        nr, nc = rng.randint(1, 9), rng.randint(1, 9)
        kind = trial % 5
        if kind == 0:
            cost = rng.randn(nr, nc)
        elif kind == 1:  # heavy ties
            cost = rng.randint(0, 3, size=(nr, nc)).astype(np.float64)
        elif kind == 2:  # constant
            cost = np.full((nr, nc), float(rng.randint(-2, 3)))
        elif kind == 3:  # float32 scores negated, as the reference builds them
            cost = (-rng.rand(nr, nc).astype(np.float32)).astype(np.float64)
        else:  # some forbidden entries but feasible (a finite diagonal band)
            cost = rng.randint(0, 4, size=(nr, nc)).astype(np.float64)
            mask = rng.rand(nr, nc) < 0.3
            for i in range(min(nr, nc)):
                mask[i, i] = False
            cost[mask] = np.inf
        _same_assignment(cost)
        n += 1
    assert n == 4000
    # larger problems
    for s in range(50):
        cost = np.random.RandomState(100 + s).randint(0, 10, size=(40, 37)).astype(np.float64)
        _same_assignment(cost)
        _same_assignment(cost.T.copy())


def test_lsap_edge_cases():
    r, c = P.linear_sum_assignment(np.zeros((0, 3)))
    assert r.size == 0 and c.size == 0
    with pytest.raises(ValueError):
        P.linear_sum_assignment(np.array([[np.inf, np.inf], [1.0, np.inf]]))  # infeasible, like scipy
    with pytest.raises(ValueError):
        scipy_lsa(np.array([[np.inf, np.inf], [1.0, np.inf]]))
    with pytest.raises(ValueError):
        P.linear_sum_assignment(np.array([[np.nan, 1.0]]))


def test_toposort_matches_reference_vectors():
    z = G.load("paf.npz")
    meta = json.loads(str(z["meta_json"]))
    for nm, t in meta["toposort"].items():
        assert list(P.toposort_edges([tuple(e) for e in t["edges"]])) == t["order"], nm
    # KAT of the reference's own test (tests/inference/test_paf_grouping.py:202-239 style): chain
    assert P.toposort_edges([(0, 1), (1, 2), (2, 3)]) == (0, 1, 2)


def _flat(lst, dtype, width=None):
    if width:
        return np.concatenate([np.asarray(a).reshape(-1, width) for a in lst]).astype(dtype)
    return np.concatenate([np.asarray(a).reshape(-1) for a in lst]).astype(dtype)


@pytest.mark.parametrize("name", ["chain5", "tree6", "chain13", "rev4"])
def test_group_batch_matches_reference_on_golden_candidates(name):
    """Feed the REFERENCE's peaks + scored candidates to the C++ matcher/assembler and compare
    with the reference's grouped instances (bit-exact membership, exact values)."""
    z = G.load("paf.npz")
    meta = json.loads(str(z["meta_json"]))["specs"][name]
    edges = [tuple(e) for e in meta["edges"]]
    n_nodes = meta["n_nodes"]
    pk, pv, pc = G.ragged(z, f"{name}/peaks"), G.ragged(z, f"{name}/vals"), G.ragged(z, f"{name}/chans")
    ce, cp, cs = G.ragged(z, f"{name}/edge_inds"), G.ragged(z, f"{name}/edge_peak_inds"), G.ragged(z, f"{name}/line_scores")
    B = len(pk)
    po = np.concatenate([[0], np.cumsum([len(a) for a in pk])]).astype(np.int32)
    co = np.concatenate([[0], np.cumsum([len(a) for a in ce])]).astype(np.int32)
    pairs = _flat(cp, np.int32, 2)
    kp, vals, scores, n_inst = P.group_batch_host(
        n_nodes, edges, _flat(pk, np.float32, 2), _flat(pv, np.float32), _flat(pc, np.int32), po, _flat(ce, np.int32), pairs[:, 0], pairs[:, 1],
        _flat(cs, np.float32), co, 0.25, 0, 32, False,
    )
    for b in range(B):
        ref = G.ragged(z, f"{name}/inst")[b].reshape(-1, n_nodes, 2)
        assert n_inst[b] == ref.shape[0]
        got = kp[b, : n_inst[b]]
        assert np.array_equal(np.isnan(got), np.isnan(ref))
        assert np.array_equal(np.nan_to_num(got), np.nan_to_num(ref))
        assert np.array_equal(np.nan_to_num(vals[b, : n_inst[b]]), np.nan_to_num(G.ragged(z, f"{name}/inst_vals")[b]))
        assert np.array_equal(scores[b, : n_inst[b]], G.ragged(z, f"{name}/inst_scores")[b])
        assert np.isnan(kp[b, n_inst[b] :]).all()


def _pack_arena(B, peak_cap, cand_cap, pk, pv, pc, po, ce, cs_, cd, sc, co):
    """The D2H arena of BottomUpLayer's GPU stage, filled on the host: [counts 2+2B | cand offsets B+1 | xy 2P | vals P | score Q | channel P | edge Q | src Q | dst Q]."""
    n_head = (2 + 2 * B) + (B + 1)
    arena = np.full(n_head + 4 * peak_cap + 4 * cand_cap, np.float32(np.nan), dtype=np.float32)  # rows beyond the counts are undefined: poison them
    ints = arena.view(np.int32)
    n, q = len(pv), len(sc)
    ints[0] = n
    ints[1 : 1 + B] = np.diff(po)
    ints[1 + B : 2 + 2 * B] = po
    ints[2 + 2 * B : n_head] = co
    o = n_head
    arena[o : o + 2 * min(n, peak_cap)] = pk.reshape(-1)[: 2 * min(n, peak_cap)]
    o += 2 * peak_cap
    arena[o : o + min(n, peak_cap)] = pv[:peak_cap]
    o += peak_cap
    arena[o : o + min(q, cand_cap)] = sc[:cand_cap]
    o += cand_cap
    ints[o : o + min(n, peak_cap)] = pc[:peak_cap]
    for k, a in enumerate((ce, cs_, cd)):
        ints[o + peak_cap + k * cand_cap : o + peak_cap + k * cand_cap + min(q, cand_cap)] = a[:cand_cap]
    return arena


@pytest.mark.parametrize("name", ["chain5", "tree6", "chain13", "rev4"])
def test_group_packed_equals_the_unpack_and_group_pair(name):
    """ph_group_packed (the one-call CPU stage of the pipelined predictor) against _finish_scoring's unpacking + group_scored_batch on the reference's golden candidates:
    max_instances None and set (truncation by score), input scale and per-frame eff_scale undo, the max_peaks_per_node guard, and the two come-back statuses
    (arena capacity exceeded, output rows too few)."""
    from sleap_nn_amd.inference.preprocess_info import PreprocInfo
    from sleap_nn_amd.inference.streaming import GroupingParams, ScoredBatch, group_scored_batch

    z = G.load("paf.npz")
    meta = json.loads(str(z["meta_json"]))["specs"][name]
    edges = [tuple(e) for e in meta["edges"]]
    n_nodes = meta["n_nodes"]
    names = [str(i) for i in range(n_nodes)]
    pk, pv, pc = _flat(G.ragged(z, f"{name}/peaks"), np.float32, 2), _flat(G.ragged(z, f"{name}/vals"), np.float32), _flat(G.ragged(z, f"{name}/chans"), np.int32)
    ce, cs_ = _flat(G.ragged(z, f"{name}/edge_inds"), np.int32), _flat(G.ragged(z, f"{name}/line_scores"), np.float32)
    pairs = _flat(G.ragged(z, f"{name}/edge_peak_inds"), np.int32, 2)
    B = len(G.ragged(z, f"{name}/peaks"))
    po = np.concatenate([[0], np.cumsum([len(a) for a in G.ragged(z, f"{name}/peaks")])]).astype(np.int32)
    co = np.concatenate([[0], np.cumsum([len(a) for a in G.ragged(z, f"{name}/edge_inds")])]).astype(np.int32)
    e32 = np.ascontiguousarray(np.asarray(edges, dtype=np.int32).reshape(-1, 2))
    peak_cap, cand_cap = len(pv) + 7, len(cs_) + 5
    arena = _pack_arena(B, peak_cap, cand_cap, pk, pv, pc, po, ce, pairs[:, 0], pairs[:, 1], cs_, co)
    p = lambda a: ctypes.c_void_p(a.ctypes.data)

    def packed(max_instances, input_scale, eff, out_cap, max_ppn=-1, arena_=arena, caps=(peak_cap, cand_cap)):
        kp = np.empty((B, out_cap, n_nodes, 2), np.float32)
        vals = np.empty((B, out_cap, n_nodes), np.float32)
        scores = np.empty((B, out_cap), np.float32)
        n_inst = np.zeros(B, np.int32)
        status = np.zeros(4, np.int32)
        L.check(L.lib().ph_group_packed(p(arena_), B, n_nodes, caps[0], caps[1], p(e32), len(edges), 0.25, 0.0, 0, -1 if max_instances is None else max_instances, max_ppn,
                                        input_scale, p(eff), out_cap, p(kp), p(vals), p(scores), p(n_inst), p(status)))
        return kp, vals, scores, n_inst, status

    for max_instances, input_scale, eff in ((None, 1.0, np.ones(B, np.float32)), (2, 0.5, np.ones(B, np.float32)), (None, 1.0, np.linspace(0.5, 1.5, B).astype(np.float32)),
                                           (1, 0.75, np.linspace(0.5, 1.5, B).astype(np.float32))):
        info = PreprocInfo(eff_scale=torch.from_numpy(eff.copy()), input_scale=input_scale)
        scored = ScoredBatch(peaks_xy=pk, peak_vals=pv, peak_channel=pc, peak_offsets=po, cand_edge=ce, cand_src=pairs[:, 0].copy(), cand_dst=pairs[:, 1].copy(), cand_score=cs_,
                             cand_offsets=co, info=info, n_samples=B, n_nodes=n_nodes)
        params = GroupingParams(paf_scorer_kwargs={"part_names": names, "edges": [(names[a], names[b]) for a, b in edges], "pafs_stride": 4}, max_instances=max_instances)
        ref = group_scored_batch(scored, params)
        out_cap = max_instances if max_instances is not None else int(np.diff(po).max())
        kp, vals, scores, n_inst, status = packed(max_instances, input_scale, eff, out_cap)
        assert status[0] == len(pv) and status[1] == len(cs_) and status[2] == 0
        mi = int(status[3])
        assert tuple(ref.pred_keypoints.shape) == (B, mi, n_nodes, 2)
        assert np.array_equal(kp[:, :mi], ref.pred_keypoints.numpy(), equal_nan=True)
        assert np.array_equal(vals[:, :mi], ref.pred_peak_values.numpy(), equal_nan=True)
        assert np.array_equal(scores[:, :mi], ref.instance_scores.numpy(), equal_nan=True)
    ones = np.ones(B, np.float32)
    # too few output rows for max_instances = None: nothing grouped, the capacity to come back with
    st = packed(None, 1.0, ones, 1)[4]
    assert (st[2] & 2) and st[3] == max(1, int(np.diff(po).max()))
    # an arena whose capacities the counts exceed
    small = _pack_arena(B, 2, 3, pk, pv, pc, po, ce, pairs[:, 0], pairs[:, 1], cs_, co)
    st = packed(None, 1.0, ones, 8, arena_=small, caps=(2, 3))[4]
    assert (st[2] & 1) and st[0] == len(pv) and st[1] == len(cs_)
    # the max_peaks_per_node guard: a frame with more peaks of one node than allowed -> a batch of NaNs
    most = max(int(np.bincount(pc[po[b] : po[b + 1]], minlength=n_nodes).max()) for b in range(B))
    kp, vals, scores, n_inst, st = packed(None, 1.0, ones, 4, max_ppn=most - 1)
    assert (st[2] & 4) and st[3] == 1 and np.isnan(kp).all() and np.isnan(scores).all()
    assert packed(None, 1.0, ones, int(np.diff(po).max()), max_ppn=most)[4][2] == 0


def test_group_batch_matches_oracle_on_random_graphs():
    """Randomised differential test vs the oracle (ties, low scores, merges, min_instance_peaks)."""
    rng = np.random.RandomState(3)
    for trial in range(200):
        n_nodes = rng.randint(2, 7)
        # random tree or chain, shuffled edge list
        edges = [(int(rng.randint(0, i)), i) for i in range(1, n_nodes)]
        rng.shuffle(edges)
        if trial % 4 == 0:
            edges = edges[: max(1, len(edges) - 1)]
        n_peaks = rng.randint(0, 14)
        chans = rng.randint(0, n_nodes, size=n_peaks).astype(np.int32)
        peaks = rng.rand(n_peaks, 2).astype(np.float32) * 100
        vals = rng.rand(n_peaks).astype(np.float32)
        e, pr = O.connection_candidates(torch.from_numpy(chans), edges, n_nodes)
        quant = trial % 3 == 0
        sc = rng.rand(e.shape[0]).astype(np.float32)
        if quant:
            sc = (np.round(sc * 4) / 4).astype(np.float32)  # exact ties
        mip = [0, 2, 0.5][trial % 3]
        try:
            m = O.match_candidates_sample(e, pr, torch.from_numpy(sc), len(edges))
            topo = O.toposort_edges(edges)
        except ValueError:
            continue
        ref = O.assemble_instances(peaks, vals, chans, *m, n_nodes, edges, topo, mip, 0.25)
        prn = pr.numpy().astype(np.int32).reshape(-1, 2)
        kp, v, s, n_inst = P.group_batch_host(
            n_nodes, edges, peaks, vals, chans, np.array([0, n_peaks], np.int32), e.numpy(), prn[:, 0], prn[:, 1], sc,
            np.array([0, e.shape[0]], np.int32), 0.25, mip, 16, False,
        )
        assert n_inst[0] == ref[0].shape[0], (trial, edges)
        assert np.array_equal(np.nan_to_num(kp[0, : n_inst[0]], nan=-1), np.nan_to_num(ref[0], nan=-1)), trial
        assert np.array_equal(np.nan_to_num(v[0, : n_inst[0]], nan=-1), np.nan_to_num(ref[1], nan=-1))
        assert np.array_equal(s[0, : n_inst[0]], ref[2])


def test_model_plan_names_and_param_count():
    from sleap_nn_amd.architectures.model import Model

    z = G.load("ckpt_bottomup.npz")
    cfg = G.config(z)
    m = Model("unet", cfg["backbone"], cfg["heads"], "bottomup")
    w = G.weights(z)
    assert set(m.param_shapes) == set(w)  # checkpoint-compatible names
    for k, v in w.items():
        assert tuple(m.param_shapes[k]) == tuple(v.shape), k
    m.load_state_dict({"model." + k: v for k, v in w.items()}, strict=True)
    with pytest.raises(RuntimeError):
        m.load_state_dict({k: v for k, v in list(w.items())[:-1]}, strict=True)
    bb = {"in_channels": 1, "kernel_size": 3, "filters": 16, "filters_rate": 2, "max_stride": 32, "stem_stride": None, "middle_block": True, "up_interpolate": True, "stacks": 1, "convs_per_block": 2, "output_stride": 4}
    heads = {"confmaps": {"part_names": [str(i) for i in range(13)], "output_stride": 4}, "pafs": {"edges": [[str(i), str(i + 1)] for i in range(12)], "output_stride": 8}}
    m3 = Model("unet", bb, heads, "bottomup")
    assert m3.num_parameters() == 7819861
    assert [h.name for h in m3.heads] == ["MultiInstanceConfmapsHead", "PartAffinityFieldsHead"]


def test_backend_protocol_and_layer_type_checks():
    from sleap_nn_amd.inference.backends import HipBackend, ModelBackend
    from sleap_nn_amd.inference.layers import PostprocessConfig, PreprocessConfig, SingleInstanceLayer

    class Fake:
        device = "cuda:0"
        does_baked_postproc = False

        def __call__(self, x):
            return {}

        def warmup(self, s):
            pass

    assert isinstance(Fake(), ModelBackend)
    with pytest.raises(TypeError):
        SingleInstanceLayer(backend=object(), output_stride=2)
    with pytest.raises(ValueError):
        PreprocessConfig(ensure_rgb=True, ensure_grayscale=True)
    assert PostprocessConfig(refinement="none").effective_refinement is None
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError):
            HipBackend(model=None)  # fails loudly without a GPU: no CPU fallback
    layer = SingleInstanceLayer(backend=Fake(), output_stride=2, max_stride=16)
    x, info = layer.preprocess(np.zeros((100, 70), dtype=np.uint8))
    assert tuple(x.shape) == (1, 1, 1, 112, 80) and info.original_size == (100, 70)
    with pytest.raises(KeyError):
        layer._extract_confmaps({"a": torch.zeros(1), "b": torch.zeros(1)})


def test_group_class_peaks_matches_oracle():
    """C++ Hungarian class matching vs the oracle (which uses SciPy, like the reference)."""
    from sleap_nn_amd.inference.ops.identity import group_class_peaks

    rng = np.random.RandomState(5)
    for trial in range(100):
        n, K, B, N = rng.randint(0, 30), rng.randint(1, 5), rng.randint(1, 4), rng.randint(1, 4)
        probs = rng.rand(n, K).astype(np.float32)
        if trial % 2:
            probs = (np.round(probs * 4) / 4).astype(np.float32)
        sb = np.sort(rng.randint(0, B, size=n)).astype(np.int32)
        sc = rng.randint(0, N, size=n).astype(np.int32)
        rp, rc = O.group_class_peaks(torch.from_numpy(probs).reshape(n, K), torch.from_numpy(sb), torch.from_numpy(sc), B, N)
        gp, gc = group_class_peaks(torch.from_numpy(probs).reshape(n, K), sb, sc, B, N)
        assert np.array_equal(rp.numpy(), gp.numpy()) and np.array_equal(rc.numpy(), gc.numpy()), trial


def test_run_directory_ingestion():
    """Lightning ``best.ckpt`` + ``training_config.yaml`` of the reference's fixture run directories
    (copied as data under tests/golden/ckpt_dirs) load without lightning / omegaconf installed."""
    from sleap_nn_amd.inference.loaders import load_model_assets

    d = os.path.join(ROOT, "tests", "golden", "ckpt_dirs", "minimal_instance_bottomup")
    a = load_model_assets(d)
    assert a.model_type == "bottomup" and a.backbone_type == "unet"
    assert a.node_names == ["A", "B"] and a.edges == [("A", "B")]
    m = a.build_model()
    z = G.load("ckpt_bottomup.npz")
    for k, v in G.weights(z).items():
        assert torch.equal(m.state_dict()[k], v), k
    s = load_model_assets(os.path.join(ROOT, "tests", "golden", "ckpt_dirs", "minimal_instance_single_instance"))
    assert s.model_type == "single_instance" and s.backbone_config["in_channels"] == 3
    with pytest.raises(FileNotFoundError):
        load_model_assets(os.path.join(ROOT, "tests"))


def test_post_inference_filters_match_reference():
    """Host-side instance filters (inference/ops/filters.py) vs the reference's own NMS / IoU / OKS helpers
    on random instance sets incl. missing nodes, all-NaN instances, near-duplicates and score ties."""
    from sleap_nn_amd.inference.ops import filters as F
    from sleap_nn_amd.inference.outputs import Outputs

    g = G.load("filters.npz")
    for c in range(int(g["n_cases"])):
        pts, scores = g[f"{c}/points"], g[f"{c}/scores"]
        boxes = np.array([F.instance_bbox(p) for p in pts])
        np.testing.assert_array_equal(boxes, g[f"{c}/bboxes"])
        np.testing.assert_allclose(F.iou_one_to_many(boxes[0], boxes), g[f"{c}/iou_row0"], rtol=0, atol=0)
        got = np.array([[F.oks(a, b) for b in pts] for a in pts])
        np.testing.assert_allclose(got, g[f"{c}/oks_matrix"], rtol=0, atol=1e-15)
        for thr in (0.1, 0.5, 0.8):
            assert F.nms_greedy(list(pts), scores, thr, "iou") == g[f"{c}/keep_iou_{thr}"].tolist()
            assert F.nms_greedy(list(pts), scores, thr, "oks") == g[f"{c}/keep_oks_{thr}"].tolist()
    # the Outputs wrapper: node-count, confidence and overlap filters in the reference's order
    pts = g["3/points"]
    n_inst, n_nodes = pts.shape[:2]
    vals = np.where(np.isnan(pts).any(-1), np.nan, 0.5)
    o = Outputs(pred_keypoints=torch.from_numpy(pts[None]).float(), pred_peak_values=torch.from_numpy(vals[None]).float(),
                instance_scores=torch.from_numpy(g["3/scores"][None]).float())
    out, keep = F.filter_outputs(o, min_visible_nodes=2, overlap_threshold=0.5, overlap_method="iou")
    nv = (~np.isnan(pts).any(-1)).sum(-1)
    cand = [i for i in range(n_inst) if nv[i] >= 2]
    sc32 = g["3/scores"].astype(np.float32).astype(np.float64)
    want = [cand[j] for j in F.nms_greedy([pts.astype(np.float32).astype(np.float64)[i] for i in cand], sc32[cand], 0.5, "iou")]
    assert keep[0] == want
    dropped = [i for i in range(n_inst) if i not in keep[0]]
    assert torch.isnan(out.pred_keypoints[0, dropped]).all() and not torch.isnan(out.instance_scores[0, keep[0]]).any()


def test_centroid_nms_matches_reference():
    """TopDownLayer._centroid_nms_mask (host logic) vs the reference's, incl. NaN slots, close pairs and ties."""
    from sleap_nn_amd.inference.layers.topdown import TopDownLayer

    g = G.load("centroid_nms.npz")
    for c in range(int(g["n_cases"])):
        layer = TopDownLayer.__new__(TopDownLayer)
        layer.crop_size = tuple(int(v) for v in g[f"{c}/crop"])
        layer.centroid_nms_threshold = float(g[f"{c}/thr"])
        cent, vals = torch.from_numpy(g[f"{c}/centroids"]), torch.from_numpy(g[f"{c}/vals"])
        valid = ~torch.isnan(cent).any(-1)
        keep = layer._centroid_nms_mask(cent, vals, valid)
        np.testing.assert_array_equal(keep.numpy(), g[f"{c}/keep"], err_msg=f"case {c}")


def test_coordinate_ladder_known_answers():
    """Replays the known-answer vectors of the reference's tests/inference/ops/test_coord.py (identity
    short-circuits return the same object; per-sample eff_scale broadcasting; crop offsets; round trip)."""
    from sleap_nn_amd.inference.ops.coord import add_crop_offset, undo_eff_scale, undo_input_scale, undo_stride

    c = torch.tensor([[1.0, 2.0], [3.0, 4.0]])
    assert undo_stride(c, 1) is c and undo_input_scale(c, 1.0) is c
    torch.testing.assert_close(undo_stride(torch.tensor([[2.0, 4.0]]), 4), torch.tensor([[8.0, 16.0]]))
    assert undo_stride(torch.zeros(3, 5, 7, 2), 2).shape == (3, 5, 7, 2)
    torch.testing.assert_close(undo_input_scale(torch.tensor([[2.0, 8.0]]), 0.5), torch.tensor([[4.0, 16.0]]))
    c3 = torch.tensor([[[1.0, 2.0], [3.0, 4.0]]])
    assert undo_eff_scale(c3, torch.ones(1)) is c3
    coords = torch.tensor([[[2.0, 4.0], [6.0, 8.0]], [[1.0, 1.0], [2.0, 2.0]]])
    torch.testing.assert_close(undo_eff_scale(coords, torch.tensor([2.0, 0.5])), torch.tensor([[[1.0, 2.0], [3.0, 4.0]], [[2.0, 2.0], [4.0, 4.0]]]))
    out = undo_eff_scale(torch.ones(2, 3, 2, 2) * 4.0, torch.tensor([2.0, 4.0]))
    torch.testing.assert_close(out[0], torch.full((3, 2, 2), 2.0))
    torch.testing.assert_close(out[1], torch.full((3, 2, 2), 1.0))
    torch.testing.assert_close(add_crop_offset(torch.tensor([[[1.0, 2.0], [3.0, 4.0]]]), torch.tensor([[10.0, 20.0]])), torch.tensor([[[11.0, 22.0], [13.0, 24.0]]]))
    torch.testing.assert_close(add_crop_offset(torch.tensor([[[1.0, 1.0], [2.0, 2.0]], [[3.0, 3.0], [4.0, 4.0]]]), torch.tensor([[100.0, 0.0], [0.0, 100.0]])),
                               torch.tensor([[[101.0, 1.0], [102.0, 2.0]], [[3.0, 103.0], [4.0, 104.0]]]))
    rng = np.random.default_rng(0)
    original = torch.tensor(rng.uniform(0, 100, size=(2, 3, 2)).astype(np.float32))
    eff = torch.tensor([2.0, 1.5])
    fwd = original * eff.view(2, 1, 1) * 0.5 / 4
    torch.testing.assert_close(undo_eff_scale(undo_input_scale(undo_stride(fwd, 4), 0.5), eff), original)


def test_unet_structure_known_answers():
    """tests/architectures/test_unet.py:20-111 of the reference: a UNet(filters 16, rate 2, max_stride 16, output_stride 1)
    + a 13-channel 1x1 head has 38 parameter tensors and 1,962,541 parameters; decoder strides / channels."""
    from sleap_nn_amd.architectures.model import Model

    bb = {"in_channels": 1, "kernel_size": 3, "filters": 16, "filters_rate": 2, "max_stride": 16, "convs_per_block": 2, "stacks": 1,
          "stem_stride": None, "middle_block": True, "up_interpolate": True, "block_contraction": False, "output_stride": 1}
    heads = {"confmaps": {"part_names": [str(i) for i in range(13)], "sigma": 5.0, "output_stride": 1}}
    m = Model("unet", bb, heads, "single_instance")
    assert len(m.param_shapes) == 38
    assert m.num_parameters() == 1962541
    assert m.backbone.decoder_stride_to_filters == {16: 256, 8: 128, 4: 64, 2: 32, 1: 16}
    sd = O.init_state(bb, heads, "single_instance")
    assert sorted(sd) == sorted(m.param_shapes) and sum(v.numel() for v in sd.values()) == 1962541


def test_winograd_f23_identity_used_by_the_conv_kernels():
    """The algebra conv3x3_wino_persist_kernel / wino_pack_kernel rely on: two neighbouring outputs of a 3-tap row
    from four multiplications, with exactly the transforms the kernels apply."""
    rng = np.random.default_rng(0)
    d = rng.standard_normal((1000, 4))
    g = rng.standard_normal((1000, 3))
    u = np.stack([g[:, 0], 0.5 * ((g[:, 0] + g[:, 2]) + g[:, 1]), 0.5 * ((g[:, 0] + g[:, 2]) - g[:, 1]), g[:, 2]], axis=1)  # wino_pack_kernel
    v = np.stack([d[:, 0] - d[:, 2], d[:, 1] + d[:, 2], d[:, 2] - d[:, 1], d[:, 1] - d[:, 3]], axis=1)  # make_a
    m = u * v
    y0 = (m[:, 0] + m[:, 1]) + m[:, 2]  # epilogue
    y1 = (m[:, 1] - m[:, 2]) - m[:, 3]
    assert np.allclose(y0, (d[:, 0:3] * g).sum(1), atol=1e-12)
    assert np.allclose(y1, (d[:, 1:4] * g).sum(1), atol=1e-12)


def test_lr_schedules_match_the_reference_and_torch():
    """training/schedulers.py: the four policies of configure_optimizers, epoch by epoch, against learning-rate sequences
    produced by the reference's own scheduler classes and torch.optim.lr_scheduler (tests/golden/schedulers.npz)."""
    from sleap_nn_amd.training.schedulers import LRSchedule
    from tests import _golden as G

    z = G.load("schedulers.npz")
    losses = z["losses"].tolist()
    cases = {
        "cosine": ({"cosine_annealing_warmup": {"warmup_epochs": 4, "max_epochs": 25, "warmup_start_lr": 1e-5, "eta_min": 1e-6}}, None),
        "cosine_nowarm": ({"cosine_annealing_warmup": {"warmup_epochs": 0, "max_epochs": None}}, 20),
        "linear": ({"linear_warmup_linear_decay": {"warmup_epochs": 5, "max_epochs": 28, "warmup_start_lr": 0.0, "end_lr": 2e-5}}, None),
        "step": ({"step_lr": {"step_size": 7, "gamma": 0.3}}, None),
        "plateau_abs": ({"reduce_lr_on_plateau": {"threshold": 1e-6, "threshold_mode": "abs", "cooldown": 3, "patience": 2, "factor": 0.5, "min_lr": 1e-8}}, None),
        "plateau_rel": ({"reduce_lr_on_plateau": {"threshold": 0.05, "threshold_mode": "rel", "cooldown": 0, "patience": 1, "factor": 0.1, "min_lr": 2e-5}}, None),
    }
    for name, (cfg, max_epochs) in cases.items():
        s = LRSchedule(1e-3, cfg, max_epochs=max_epochs)
        got = [s.lr] + [s.step(losses[e]) for e in range(30)]
        assert np.allclose(got, z[name], rtol=1e-12, atol=0), (name, got[:8], z[name][:8])
    # priority when several are set, and the constant default
    s = LRSchedule(1e-3, {"step_lr": {"step_size": 1, "gamma": 0.5}, "cosine_annealing_warmup": {"warmup_epochs": 0, "max_epochs": 10}, "reduce_lr_on_plateau": {}})
    assert s.kind == "cosine_annealing_warmup"
    s = LRSchedule(2e-4, None)
    assert [s.step() for _ in range(3)] == [2e-4] * 3


def test_host_grouping_under_sanitizers(tmp_path):
    """The host half of the hot path (csrc/group_host.cpp: assignment, toposort, assembly, class grouping) compiled ALONE by g++ with
    AddressSanitizer + UndefinedBehaviorSanitizer and driven through the same differential tests as the product library (scipy ties,
    the reference's golden candidates, 200 random graphs with empty / ragged inputs): any out-of-bounds access, use-after-free or
    undefined arithmetic aborts the child.  (GPU sanitizers are not available on this pool; the device kernels have their own
    bounds reasoning and the repeatability screen of tools/race_screen.py.)"""
    import shutil
    import subprocess
    import sys

    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    asan = subprocess.run([gxx, "-print-file-name=libasan.so"], capture_output=True, text=True).stdout.strip()
    if not os.path.isabs(asan) or not os.path.exists(asan):
        pytest.skip("no libasan")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    so = str(tmp_path / "libgroup_san.so")
    r = subprocess.run([gxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-fPIC",
                        "-shared", os.path.join(root, "sleap_nn_amd", "csrc", "group_host.cpp"), os.path.join(root, "tests", "san_stub.cpp"), "-o", so],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    env = dict(os.environ, LD_PRELOAD=asan, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1")  # the interpreter itself "leaks" by design
    r = subprocess.run([sys.executable, os.path.join(root, "tests", "sanitize_host.py"), so], capture_output=True, text=True, env=env, timeout=900, cwd=root)
    assert r.returncode == 0 and "sanitized host grouping: OK" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])


def _recording_sleap_io():
    """A stand-in for the `sleap_io` package (absent from this image): records what the packaging code hands it."""
    import types

    class PredictedInstance:
        def __init__(self, **kw):
            self.__dict__.update(kw)

        @classmethod
        def from_numpy(cls, points_data, point_scores=None, score=0.0, skeleton=None, track=None, tracking_score=None):
            return cls(points=np.array(points_data, dtype=np.float32), point_scores=np.array(point_scores, dtype=np.float32), score=float(score),
                       skeleton=skeleton, track=track, tracking_score=tracking_score)

    class LabeledFrame:
        def __init__(self, video=None, frame_idx=0, instances=(), **extra):
            self.video, self.frame_idx, self.instances = video, int(frame_idx), list(instances)
            assert all(not v for v in extra.values())  # pose outputs carry no centroids / masks / rois objects

    class Labels:
        def __init__(self, labeled_frames=(), videos=(), skeletons=()):
            self.labeled_frames, self.videos, self.skeletons, self.tracks = list(labeled_frames), list(videos), list(skeletons), []

    class Skeleton:
        def __init__(self, nodes):
            self.nodes = list(nodes)

    class Track:
        def __init__(self, name):
            self.name = name

    m = types.ModuleType("sleap_io")
    m.PredictedInstance, m.LabeledFrame, m.Labels, m.Skeleton, m.Track = PredictedInstance, LabeledFrame, Labels, Skeleton, Track
    return m


def _outputs_cases():
    """The Outputs of every packaging case of test_outputs_to_instances_and_to_labels (oracle/gen_golden.py::outputs_packaging_fixture hands the same to the reference)."""
    nan = float("nan")
    kp = torch.tensor([[[[1.0, 2.0], [3.0, 4.0], [nan, nan]], [[nan, nan]] * 3, [[5.0, 6.0], [nan, nan], [7.0, 8.0]]],
                       [[[nan, nan]] * 3] * 3])
    pv = torch.tensor([[[0.9, 0.8, nan], [nan, nan, nan], [0.5, nan, 0.25]], [[nan] * 3] * 3])
    cases = {
        "bottomup": dict(pred_keypoints=kp, pred_peak_values=pv, instance_scores=torch.tensor([[2.5, nan, 1.5], [nan, nan, nan]]),
                         frame_indices=torch.tensor([7, 8]), video_indices=torch.tensor([1, 0])),
        "single_instance": dict(pred_keypoints=kp[:, :1], pred_peak_values=pv[:, :1]),
        "multiclass_topdown": dict(pred_keypoints=kp, pred_peak_values=pv, instance_scores=torch.tensor([[0.7, nan, 0.6], [nan] * 3]),
                                   pred_class_inds=torch.tensor([[[1] * 3, [-1] * 3, [0] * 3], [[-1] * 3] * 3]),
                                   instance_tracking_scores=torch.tensor([[0.95, nan, 0.85], [nan] * 3])),
        "multiclass_bottomup": dict(pred_keypoints=kp, pred_peak_values=pv, instance_scores=torch.tensor([[0.7, nan, 0.6], [nan] * 3]),
                                    instance_tracking_scores=torch.tensor([[0.4, nan, 0.3], [nan] * 3])),
        "centroid_only": dict(pred_centroids=torch.tensor([[[10.0, 20.0], [nan, nan], [30.0, 40.0]], [[nan, nan]] * 3]),
                              pred_centroid_values=torch.tensor([[0.8, nan, nan], [nan] * 3])),
    }
    return cases


def _packaging_record(instances, skel, tracks):
    """Instances as plain data (NaN as None, the track by its index in `tracks`): the form tests/golden/outputs_packaging.json holds the reference's in."""
    def num(a):
        a = np.asarray(a, dtype=np.float64) if a is not None else None
        return None if a is None else [num(x) for x in a] if a.ndim else (None if np.isnan(a) else float(a))

    return [{"points": num(i.points), "point_scores": num(i.point_scores), "score": num(i.score), "skeleton_given": i.skeleton is skel,
             "track": None if i.track is None else tracks.index(i.track), "tracking_score": num(i.tracking_score)} for i in instances]


def _packaging_run(outputs_cls, sio):
    """Every case through `outputs_cls` (the product's Outputs or the reference's) with the recording stand-in `sio`: per case the instances of
    frames 0 and 1 and what to_labels packs (frame indices, videos, track names)."""
    skel = sio.Skeleton(["a", "b", "c"])
    tracks = [sio.Track("t0"), sio.Track("t1"), sio.Track("t2")]
    videos = ["video0", "video1"]
    rec = {}
    for name, kw in _outputs_cases().items():
        o = outputs_cls(**kw)
        tr = tracks if name.startswith("multiclass") else None
        anchor = 1 if name == "centroid_only" else None
        lab = o.to_labels(skel, videos=videos if name == "bottomup" else None, anchor_ind=anchor, tracks=tr)
        rec[name] = {"instances": [_packaging_record(o.to_instances(skel, b, anchor_ind=anchor, tracks=tr), skel, tracks) for b in range(2)],
                     "labels": {"frame_idx": [f.frame_idx for f in lab.labeled_frames], "video": [f.video for f in lab.labeled_frames], "tracks": [t.name for t in lab.tracks]}}
    return rec


def test_outputs_to_instances_and_to_labels(monkeypatch):
    """`Outputs.to_instances` / `to_labels` (outputs.py:284-477, 612-779) on a recording stand-in for sleap_io: NaN slots dropped,
    per-instance score = instance_scores or the nansum of the node scores, centroid-only packaging at the anchor node, multi-class
    tracks by class index (top-down) or by slot (bottom-up), frame / video indices, loud on a missing video -- and identical to what
    the reference's own methods return on the same tensors (tests/golden/outputs_packaging.json)."""
    import sys

    from sleap_nn_amd.inference.outputs import Outputs

    sio = _recording_sleap_io()
    monkeypatch.setitem(sys.modules, "sleap_io", sio)
    skel = sio.Skeleton(["a", "b", "c"])
    cases = _outputs_cases()
    kp, pv = cases["bottomup"]["pred_keypoints"], cases["bottomup"]["pred_peak_values"]
    tracks = [sio.Track("t0"), sio.Track("t1"), sio.Track("t2")]
    videos = ["video0", "video1"]
    for name, kw in cases.items():
        o = Outputs(**kw)
        tr = tracks if name.startswith("multiclass") else None
        got = [o.to_instances(skel, b, anchor_ind=1 if name == "centroid_only" else None, tracks=tr) for b in range(2)]
        if name == "bottomup":
            assert [len(g) for g in got] == [2, 0] and got[0][0].score == 2.5 and got[0][1].score == 1.5
            assert np.isnan(got[0][0].points[2]).all() and got[0][1].point_scores[2] == 0.25
        if name == "single_instance":
            assert len(got[0]) == 1 and abs(got[0][0].score - 1.7) < 1e-6 and got[1] == []  # nansum of the node scores
        if name == "multiclass_topdown":
            assert [i.track.name for i in got[0]] == ["t1", "t0"] and [i.tracking_score for i in got[0]] == [pytest.approx(0.95), pytest.approx(0.85)]
        if name == "multiclass_bottomup":
            assert [i.track.name for i in got[0]] == ["t0", "t2"]  # the instance slot IS the class
        if name == "centroid_only":
            assert len(got[0]) == 2 and np.array_equal(got[0][0].points[1], [10.0, 20.0]) and np.isnan(got[0][0].points[[0, 2]]).all()
            assert got[0][0].score == pytest.approx(0.8) and got[0][1].score == 0.0 and np.isnan(got[0][1].point_scores).all()
            one = sio.Skeleton(["centroid"])
            col = o.to_instances(skel, 0, collapse_skeleton=one)
            assert len(col) == 2 and col[0].skeleton is one and col[0].points.shape == (1, 2)
        lab = o.to_labels(skel, videos=videos if name == "bottomup" else None, anchor_ind=1 if name == "centroid_only" else None, tracks=tr)
        assert len(lab.labeled_frames) == 1 and lab.skeletons == [skel]
        if name == "bottomup":
            f = lab.labeled_frames[0]
            assert f.frame_idx == 7 and f.video == "video1" and lab.videos == videos
        if tr is not None:
            assert [t.name for t in lab.tracks] == sorted({i.track.name for i in lab.labeled_frames[0].instances}, key=[i.track.name for i in lab.labeled_frames[0].instances].index)
        assert len(o.to_labels(skel, keep_empty_frames=True).labeled_frames) == 2
    with pytest.raises(IndexError):
        Outputs(pred_keypoints=kp, pred_peak_values=pv, video_indices=torch.tensor([2, 0])).to_labels(skel, videos=videos)
    with pytest.raises(ValueError):
        Outputs(**cases["centroid_only"]).to_instances(skel, 0, anchor_ind=5)
    assert Outputs().to_instances(skel) == []
    with open(os.path.join(G.GOLDEN_DIR, "outputs_packaging.json")) as f:
        assert _packaging_run(Outputs, sio) == json.load(f)


def test_wino4_transform_tables_known_answer():
    """The arithmetic conv3x3_wino4_kernel implements -- F(4x4,3x3) with the kernel's own operation order (three-operation row chains, the
    14-operation column pass, the A^T passes) and the bilinear x2 of the second source folded into the input transform (B^T U as four row
    coefficients, clamped low-resolution indices, zero padding of the up-sampled tensor at every image border) -- restated in numpy
    (tools/proto/wino4_math.py) against torch's conv2d over the concatenated, torch-up-sampled input."""
    import importlib.util

    spec = importlib.util.spec_from_file_location("wino4_math", os.path.join(ROOT, "tools", "proto", "wino4_math.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    for seed in (0, 1):
        err_fold, err_plain = mod.check(seed)
        assert err_plain <= 1e-12          # float64 restatement: exact up to rounding
        assert err_fold <= 5e-7            # (torch's interpolate runs in float32)


def test_split_k_plan_known_answers():
    """The routing arithmetic of the small-batch regime (pure host code: wino2d_ksplit_shape / wino4_ksplit_shape through ph_debug_split_plan), on a 256-CU chip.
    F(2x2,3x3): split only when the layer's (16 x 16 tile, N tile) units fill less than half of the CUs and K has >= 8 halves; slices = min(CUs / units, halves / 3).
    F(4x4,3x3): units of 32 x 16 pixels, K >= 128 channels, slices = min(CUs / units, quarters / 16).  Half-empty N tiles (32 mod 64 channels) never split on F(2x2,3x3);
    a forced count is capped by the K granularity."""
    import ctypes as C

    def plan(B, H, W, cin, cout, splitk=1, n_cu=256):
        out = (C.c_int64 * 4)()
        assert L.lib().ph_debug_split_plan(B, H, W, cin, cout, splitk, n_cu, out) == 0
        return list(out)

    # cfg1's stride-16 level: one 16 x 16 tile x 4 N tiles, K = 256 channels = 32 halves / 64 quarters
    assert plan(1, 16, 16, 256, 256)[:2] == [10, 4]
    assert plan(1, 16, 16, 256, 256)[2] == 10 * 16 * 16 * 256 * 4 // 1024
    # cfg1's decoder concat at 32 x 32: 384 -> 128: 4 tiles x 2 N tiles = 8 units, 48 halves -> min(32, 16)
    assert plan(1, 32, 32, 384, 128)[0] == 16
    # cfg3 at 32 frames: every layer fills the chip -- no split on either kernel
    assert plan(32, 64, 64, 768, 256)[:2] == [1, 1] and plan(32, 64, 64, 768, 256)[2:] == [0, 0]
    # cfg3 at 4 frames per rank, 768 -> 256 at 64 x 64: F(2x2,3x3) has 256 units (full), F(4x4,3x3) 128 -> two slices of 96 quarters
    assert plan(4, 64, 64, 768, 256)[:2] == [1, 2]
    # fewer than 8 halves of K, or 32 output channels mod 64 (the half-empty-N-tile instantiation): no split; option 0: never; forced counts are capped
    assert plan(1, 64, 64, 32, 64)[0] == 1 and plan(1, 16, 16, 256, 96)[0] == 1 and plan(1, 16, 16, 256, 256, splitk=0)[:2] == [1, 1]
    assert plan(1, 16, 16, 64, 64, splitk=100)[0] == 8 and plan(32, 64, 64, 768, 256, splitk=3)[:2] == [3, 3]
    # a map that is no multiple of 4 cannot run on the F(4x4,3x3) kernel at all
    assert plan(1, 18, 18, 256, 256)[1] == 1


def test_hot_conv_kernels_keep_their_registers(tmp_path):
    """The F(4x4,3x3) kernel's loop lives within 256 registers per wave only because of how its source is written (an uninitialised register pair once made
    the allocator spill 144 registers of the folded-bilinear instantiation: +7 % time, no test failing).  Compile it for gfx950 (no GPU needed) and hold every
    instantiation to a small spill count -- what is left are tile-invariant values parked across the K loop -- and (next to) no scratch access inside a quarter loop."""
    import re
    import shutil
    import subprocess

    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    src = os.path.join(ROOT, "sleap_nn_amd", "csrc", "wino4_kernels.hip")
    out = tmp_path / "wino4.s"
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I", os.path.join(ROOT, "include"), "-I", os.path.dirname(src), "-S", "--cuda-device-only", "-o", str(out), src],
                   check=True, capture_output=True, timeout=600)
    text = out.read_text()
    seen = 0
    for m in re.finditer(r"^(_ZN2ph20conv3x3_wino4_kernel\w+):(.*?)s_endpgm", text, re.S | re.M):
        name, body = m.group(1), m.group(2).split("\n")
        # a quarter loop: from its header to the barrier that ends the quarter (+ the loop's closing instructions)
        inside, loops = 0, 0
        for h in [i for i, l in enumerate(body) if "Inner Loop Header: Depth=2" in l]:
            j = h
            while j < len(body) and "s_barrier" not in body[j]:
                j += 1
            if any("v_mfma" in l for l in body[h:j]):
                loops += 1
                inside += sum("scratch_" in l for l in body[h:j + 8])
        assert loops >= 4 and inside <= 2, f"{name}: {inside} scratch accesses inside {loops} quarter loops"  # (one reload sits in one of the folded-bilinear loops today)
        seen += 1
    assert seen == 4
    spills = {m.group(1): int(m.group(2)) for m in re.finditer(r"\.name:\s+(_ZN2ph20conv3x3_wino4_kernel\w+).*?\.vgpr_spill_count:\s+(\d+)", text, re.S)}
    assert len(spills) == 4 and max(spills.values()) <= 40, spills


def test_unverified_stream_lanes_warn_once_per_process():
    """when the overlap of the predictor's lanes cannot be verified (no torch.cuda._sleep, or every candidate stream queued behind a chosen
    lane) the multi-lane predictor silently loses up to a third of its throughput -- now a RuntimeWarning says so, once."""
    import warnings

    from sleap_nn_amd.inference import predictor as P

    P._lane_warning_given[0] = False
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        P._warn_unverified_lanes(3, "the probe is unavailable")
        P._warn_unverified_lanes(2, "again")
    assert len(w) == 1 and issubclass(w[0].category, RuntimeWarning) and "3 concurrent HIP streams" in str(w[0].message) and "serialise" in str(w[0].message)
    P._lane_warning_given[0] = False
