"""Fragment merge on the GPU: ``ph_seg_merge_tables`` (csrc/seg_merge_kernels.hip) behind ``group_instances_from_offsets(merge_fragments=True)`` against
the reference's recorded results -- every mask, centre, score and count equal, every affinity within 1e-7 --, the C ABI against ``merge_tables_host`` on
seeded random label maps, the capacity retries, run-to-run and stream-to-stream identity (moments included), the argument checks, a run directory
through ``Predictor``, and ``merge_fragments=False`` against the unmerged goldens.  Goldens: tools/gen_seg_merge_golden.py.

Tolerance of the moments against ``merge_tables_host``: both add the same float64 terms ``v_i`` (``rx`` is one rounded sum of an integer and a float32, the
same on both sides; a square may be fused into its addition on the device: one rounding less) in different orders.  Any order's error is at most
``(N - 1) u sum |v_i|`` with ``u = 2^-53``, so the two differ by at most ``2 N u sum |v_i|``, plus ``N u sum |v_i|`` for the fused squares: the bound used
is ``4 N u sum |v_i|`` -- derived, not measured.  Contact counts, edge order and ridge minima are exact."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests import _golden as G
from tests.test_segmentation_cpu import GROUP_NAMES as PLAIN_NAMES
from tests.test_segmentation_cpu import _case as plain_case, check_grouping, group_kwargs
from tests.test_seg_merge_cpu import MG, NAMES, RANDOM_MAPS, case, check_merged, check_rundir, merge_kwargs, random_maps_for

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0**-53


def _group(name, method=None, **kw):
    from sleap_nn_amd.inference.ops.segmentation import group_instances_from_offsets

    (fg, hm, off), p = case(name)
    trace = []
    g = group_instances_from_offsets(fg.to(DEV), hm.to(DEV), off.to(DEV), **group_kwargs(p), **merge_kwargs(p, method), merge_trace=trace, **kw)
    return g, p, trace


@pytest.mark.parametrize("name", NAMES)
def test_device_merge_reproduces_reference(name):
    """Default capacities: 'many_centres' comes back once for two-byte labels.  Prints the largest affinity difference from the recorded reference edges."""
    _p = case(name)[1]
    worst = []
    for method in sorted({"greedy", "multicut", _p["merge_method"]}):
        g, p, trace = _group(name, method)
        check_merged(name, g, p, method, trace, worst=worst)
        assert g.labels.dtype == (np.int8 if max(len(MG[f"group/{name}/{b}/peaks"]) for b in range(g.labels.shape[0])) <= 127 else np.int16)
    print(name, "largest |affinity - reference|:", max(worst, default=0.0))


def _tables_abi(lab, hm, off, cen, n, d, label_dtype, stride=2, edge_cap=None, mc=None, stream=None):
    """``ph_seg_merge_tables`` on one frame through the C ABI (outputs pre-filled with a pattern): (moments (n, 4), edges (E, 4), ridge (E,), true edge count)."""
    from sleap_nn_amd import _lib as L

    h, w = lab.shape
    mc = n if mc is None else mc
    edge_cap = max(1, n * (n - 1) // 2) if edge_cap is None else edge_cap
    lt = torch.from_numpy(lab.astype(label_dtype))[None].to(DEV)
    hm_d, off_d = torch.from_numpy(hm)[None, None].to(DEV), torch.from_numpy(off)[None].to(DEV)
    cen_d = torch.full((1, mc, 2), -9, dtype=torch.int32, device=DEV)
    cen_d[0, :n] = torch.from_numpy(cen[:n]).to(DEV)
    counts = torch.tensor([n, 0], dtype=torch.int32, device=DEV)
    mom = torch.full((1, mc, 4), -3.0, dtype=torch.float64, device=DEV)
    ecount = torch.full((1,), -5, dtype=torch.int32, device=DEV)
    edges = torch.full((1, edge_cap, 5), -7, dtype=torch.int32, device=DEV)
    need = int(L.lib().ph_seg_merge_scratch_bytes(1, h, w, mc))
    scratch = torch.full(((need + 7) // 8,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device=DEV)
    p = lambda t: C.c_void_p(t.data_ptr())
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream(DEV))  # (the buffers above were filled on the current stream)
    with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream(DEV)):
        L.check(L.lib().ph_seg_merge_tables(p(lt), p(hm_d), p(off_d), 1, h, w, stride, d, p(cen_d), p(counts), mc, lt.element_size(), p(mom), p(ecount), p(edges), edge_cap,
                                            p(scratch), need, L.current_stream_ptr()))
    torch.cuda.synchronize()
    total = int(ecount.item())
    e = edges[0].cpu().numpy()
    kept = min(total, edge_cap)
    assert np.all(e[kept:] == -7)  # nothing is written beyond the count or the capacity
    m = mom[0].cpu().numpy()
    assert not m[n:].any()
    return m[:n], e[:kept, :4].astype(np.int64), e[:kept, 4].copy().view(np.float32), total


@pytest.mark.parametrize("name,lab,n,d", RANDOM_MAPS, ids=[m[0] for m in RANDOM_MAPS])
def test_tables_equal_host_on_random_label_maps(name, lab, n, d):
    from sleap_nn_amd.inference.ops.segmentation_merge import merge_tables_host

    hm, off, cen = random_maps_for(lab, n)
    _T, ref_mom, ref_edges, ref_ridge = merge_tables_host(lab, hm, off, cen, n, 2, d)
    terms = np.zeros((n, 4))  # sum |v_i| and N per label, for the bound on the moments
    count = np.zeros(n)
    for k in range(n):
        ys, xs = np.nonzero(lab == k)
        rx = ((xs - int(cen[k][0])) * 2).astype(np.float64) + off[0][ys, xs].astype(np.float64)
        ry = ((ys - int(cen[k][1])) * 2).astype(np.float64) + off[1][ys, xs].astype(np.float64)
        terms[k], count[k] = (np.abs(rx).sum(), np.abs(ry).sum(), (rx * rx).sum(), (ry * ry).sum()), len(ys)
    for dt in ([np.int8] if n <= 127 else []) + [np.int16, np.int32]:
        mom, edges, ridge, total = _tables_abi(lab, hm, off, cen, n, d, dt)
        assert total == len(ref_edges) and np.array_equal(edges, ref_edges), (name, dt)  # contact counts and edge order
        assert np.array_equal(ridge.view(np.int32), ref_ridge.view(np.int32)), (name, dt)  # bit-equal
        err = np.abs(mom - ref_mom)
        print(name, dt.__name__, "largest moment difference / bound:", float((err / np.maximum(4 * count[:, None] * U * terms, 1e-300)).max(initial=0)))
        assert np.all(err <= 4 * count[:, None] * U * terms), (name, dt)


def test_tables_report_the_true_edge_count_beyond_the_capacity():
    from sleap_nn_amd.inference.ops.segmentation_merge import merge_tables_host

    name, lab, n, d = RANDOM_MAPS[2]
    hm, off, cen = random_maps_for(lab, n)
    _T, _m, ref_edges, ref_ridge = merge_tables_host(lab, hm, off, cen, n, 2, d)
    assert len(ref_edges) > 5
    _mom, edges, ridge, total = _tables_abi(lab, hm, off, cen, n, d, np.int8, edge_cap=5, mc=100)  # (and a record wider than the centre count)
    assert total == len(ref_edges) and np.array_equal(edges, ref_edges[:5]) and np.array_equal(ridge, ref_ridge[:5])


def test_retry_on_small_capacities():
    """An edge list, a candidate list and a label width that are too small: each comes back with room."""
    for kw in (dict(edge_cap=16), dict(edge_cap=1, cap=16, max_centers=8)):
        g, p, trace = _group("many_centres", **kw)
        check_merged("many_centres", g, p, "greedy", trace)
    g, p, trace = _group("chain", "multicut", edge_cap=2)
    check_merged("chain", g, p, "multicut", trace)


@pytest.mark.parametrize("name", ["noisy_offsets", "many_centres", "batch4"])
def test_repeatable_and_on_another_stream(name):
    g0, p, t0 = _group(name)
    s = torch.cuda.Stream(DEV)
    with torch.cuda.stream(s):
        g1, _, t1 = _group(name)
    g2, _, t2 = _group(name)
    check_merged(name, g1, p, p["merge_method"], t1)
    for g, t in ((g1, t1), (g2, t2)):
        assert np.array_equal(g0.labels, g.labels) and g0.members == g.members
        for b in range(len(g0.centers)):
            assert np.array_equal(g0.centers[b], g.centers[b]) and np.array_equal(g0.scores[b], g.scores[b]) and np.array_equal(g0.counts[b], g.counts[b])
            assert t0[b].get("edges") == t[b].get("edges") and t0[b].get("detail") == t[b].get("detail")  # affinities bit for bit: the moments are


def test_moments_are_bit_identical_between_runs_and_streams():
    name, lab, n, d = RANDOM_MAPS[1]
    hm, off, cen = random_maps_for(lab, n)
    first = _tables_abi(lab, hm, off, cen, n, d, np.int8)
    again = _tables_abi(lab, hm, off, cen, n, d, np.int8)
    other = _tables_abi(lab, hm, off, cen, n, d, np.int8, stream=torch.cuda.Stream(DEV))
    for r in (again, other):
        assert np.array_equal(first[0].view(np.int64), r[0].view(np.int64)) and np.array_equal(first[1], r[1]) and np.array_equal(first[2].view(np.int32), r[2].view(np.int32))


def test_c_abi_rejects_bad_arguments():
    from sleap_nn_amd import _lib as L

    t = torch.zeros(1 << 16, dtype=torch.int32, device=DEV)
    p = C.c_void_p(t.data_ptr())
    lib = L.lib()
    args = lambda d=1, mc=8, lb=1, sb=1 << 18, sp=p, first=p, w=4: (first, p, p, 1, 4, w, 2, d, p, p, mc, lb, p, p, p, 4, sp, sb, None)
    assert lib.ph_seg_merge_tables(*args(first=None)) == L.PH_E_INVALID  # null pointer
    assert lib.ph_seg_merge_tables(*args(mc=200, lb=1)) == L.PH_E_INVALID  # 200 centres in one-byte labels
    assert lib.ph_seg_merge_tables(*args(mc=40000, lb=2)) == L.PH_E_INVALID
    assert lib.ph_seg_merge_tables(*args(d=0)) == L.PH_E_INVALID and lib.ph_seg_merge_tables(*args(d=5)) == L.PH_E_INVALID
    assert lib.ph_seg_merge_tables(*args(w=40000)) == L.PH_E_INVALID  # a side beyond 32767
    assert lib.ph_seg_merge_tables(*args(sp=C.c_void_p(t.data_ptr() + 4))) == L.PH_E_INVALID  # unaligned scratch
    assert lib.ph_seg_merge_tables(*args(sb=8)) == L.PH_E_INVALID  # short scratch


def test_run_directory_through_predictor():
    import json

    from sleap_nn_amd.inference.layers import MergeSegmentationLayer
    from sleap_nn_amd.inference.predictor import Predictor

    rp = json.loads(str(MG["rundir/params"]))
    pred = Predictor.from_model_paths([os.path.join(G.GOLDEN_DIR, "ckpt_dirs", "tiny_bottomup_segmentation")], device=DEV, batch_size=2, merge_fragments=True,
                                      merge_thresholds=tuple(rp["merge_thresholds"]))
    assert isinstance(pred.layer, MergeSegmentationLayer)
    outs = pred.predict(MG["rundir/frames"])
    assert len(outs) == 1
    check_rundir(outs[0].pred_masks)  # (the generator asserted an empty uncertain set and all merge margins, and a merge: no pixel is excused)


@pytest.mark.parametrize("name", PLAIN_NAMES)
def test_merge_off_is_the_recorded_unmerged_result(name):
    from sleap_nn_amd.inference.ops.segmentation import group_instances_from_offsets

    (fg, hm, off), p = plain_case(name)
    g = group_instances_from_offsets(fg.to(DEV), hm.to(DEV), off.to(DEV), merge_fragments=False, **group_kwargs(p))
    assert g.members is None and g.holes is None
    check_grouping(name, g, p)
