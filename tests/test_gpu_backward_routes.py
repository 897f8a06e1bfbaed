"""Every route of the reverse sweep (csrc/backward.hip) pinned to float64, one tiny training step per case of tests/_backward_cases.py.

Per case: the options are set, one ``forward_backward`` runs, every ``must`` entry is looked up in ``last_backward_routes()`` (the record the sweep writes where it
decides; no predicate is restated here), then the loss and every parameter gradient meet two yardsticks, both the project's:
  * the fp32 oracle: loss at rtol 1e-5 / atol 1e-6, every gradient within 1e-4 of its tensor's largest magnitude (``_check_grads`` of tests/test_gpu_training.py);
  * the same oracle in float64: per tensor ``e_hip <= max(floor, 2 e_ref)``, ``e_ref`` being torch-fp32's own distance from float64 (the rule of
    test_backward_cfg3_network_with_interior_tiles), with the case's floor of the table (4 x the measured worst, at most 1e-4).
A second step must leave bitwise the same gradients and the same record.  The closure test holds the table complete: the routes seen over all cases are all there are."""
import numpy as np
import pytest
import torch

from sleap_nn_amd import _lib as L
from tests import _backward_cases as T

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# Values of the record no program of the front end reaches, each with its reason.  Anything else the record can hold must be seen in some case.
UNREACHED = {
    ("dgrad", L.KV_WINO2D_KS): "conv3x3_dgrad hands the data-gradient conv no split-K scratch (ConvArgs::split_scratch stays null), so the route never splits K",
}
_SEEN = {}  # case name -> route words of its first step (filled by test_case, read by the closure test)


def _run(case):
    sd, img, targets, lw = T.inputs(case)
    tm = T.module(case, DEV)
    dev_t = {k: v.to(DEV) for k, v in targets.items()}
    loss = tm.forward_backward(img.to(DEV), dev_t).cpu().numpy()
    torch.cuda.synchronize()
    return tm, img, dev_t, loss


@pytest.mark.parametrize("name", [c.name for c in T.CASES])
def test_case(name):
    case = T.BY_NAME[name]
    tm, img, dev_t, loss = _run(case)
    routes = tm.model.last_backward_routes()
    ops = tm.model.ops
    _SEEN[name] = list(routes)
    assert len(routes) == len(ops)
    for sel, part, field, value in case.must:
        hit = [i for i, (o, w) in enumerate(zip(ops, routes)) if T.matches(o, sel) and T.field_of(w, part, field) == value]
        assert hit, (sel, part, field, value, [L.br_decode(w) for o, w in zip(ops, routes) if T.matches(o, sel)])
    if case.frozen:
        n = tm.model.backbone.encoder_ops()
        assert n > 0 and routes[:n] == [0] * n and any(routes[n:])
    else:  # every op with parameters reports a step
        assert all(w != 0 for o, w in zip(ops, routes) if o.weight and o.kind in (L.OP_CONV, L.OP_INPUT_CONV, L.OP_CONVT, L.OP_LINEAR, L.OP_PATCH_CONV, L.OP_PATCH_STEM))
    kernels = tm.model.last_backward_kernels()  # (that record keeps its values: nothing for conv, pool, head and upsample steps)
    assert all(k == L.KV_NONE for o, k in zip(ops, kernels) if o.kind in (L.OP_CONV, L.OP_POOL, L.OP_HEAD, L.OP_UPSAMPLE))

    got = tm.named_grads()
    l32, g32 = T.reference(case, False)
    _l64, g64 = T.reference(case, True)
    assert set(got) == set(g32) == set(g64)
    want = np.array(l32, dtype=np.float32)
    assert np.allclose(loss[: len(want)], want, rtol=1e-5, atol=1e-6), (loss, l32)
    e32 = {k: float((got[k] - r).abs().max()) / max(float(r.abs().max()), 1e-12) for k, r in g32.items()}
    e_hip, e_ref = T.e_rel(got, g64), T.e_rel(g32, g64)
    worst = max(e_hip, key=e_hip.get)
    print(f"{name}: worst e_hip {e_hip[worst]:.3e} ({worst}, e_ref {e_ref[worst]:.2e}); worst against fp32 {max(e32.values()):.3e}; floor {case.floor:.1e}")
    for k in g64:
        assert e32[k] <= 1e-4, (k, e32[k])
        assert e_hip[k] <= max(case.floor, 2.0 * e_ref[k]), (k, e_hip[k], e_ref[k])

    g1 = tm.grads.clone()
    tm.forward_backward(img.to(DEV), dev_t)
    torch.cuda.synchronize()
    assert torch.equal(g1, tm.grads)
    assert tm.model.last_backward_routes() == routes
    tm.close()


def test_the_table_reaches_every_route():
    """The union over the table of weight-gradient routes, data-gradient routes and mask / bias origins is everything the record can name, but for ``UNREACHED``.
    A route added to the sweep without a case (or a case that stops reaching its route) fails here."""
    for c in T.CASES:  # (run alone, this test takes the steps itself)
        if c.name not in _SEEN:
            tm, *_ = _run(c)
            _SEEN[c.name] = tm.model.last_backward_routes()
            tm.close()
    seen = {"wgrad": set(), "dgrad": set(), "mask": set(), "bias": set(), "accumulate": set()}
    flags = {f: set() for f in L.BR_FLAGS}
    for words in _SEEN.values():
        for w in words:
            d = L.br_decode(w)
            for p in (0, 1):
                seen["wgrad"].add(d["wgrad"][p])
                seen["dgrad"].add(d["dgrad"][p])
                seen["accumulate"].add(d["accumulate"][p])
            seen["mask"].add(d["mask"])
            seen["bias"].add(d["bias"])
            for f in L.BR_FLAGS:
                flags[f].add(d[f])
    every = {"wgrad": set(L.BR_WG_NAMES), "dgrad": set(L.BR_DG_NAMES) | set(L.BR_DG_DMA_CODES), "mask": set(L.BR_MASK_NAMES), "bias": set(L.BR_BIAS_NAMES), "accumulate": {0, 1}}
    for field, values in every.items():
        unreached = {v for (f, v) in UNREACHED if f == field}
        assert seen[field] - values == set(), (field, seen[field] - values)  # nothing the binding cannot name
        assert values - seen[field] == unreached, (field, sorted(values - seen[field]), sorted(unreached))
    assert all(v == {0, 1} for v in flags.values()), flags
