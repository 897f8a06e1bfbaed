"""The route of the exact-fp32 3x3 conv (csrc/conv3x3_route.h) held to the record of the predicates it replaced (tests/golden/conv3x3_routes.json).  No GPU.

The golden was recorded once, on an MI355X, from the routing predicates as they stood before they were folded into ``conv3x3_route``; ``ph_debug_conv3x3_route`` runs the
pure function with the CU count of that record.  Every case is compared, property bits included."""
import ctypes as C
import hashlib
import json
import os
import re
from collections import Counter

import pytest

from sleap_nn_amd import _lib as L
from tests import _conv_routes as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(ROOT, "tests", "golden", "conv3x3_routes.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def cases():
    return R.cases()


def _routes(cases, n_cu, salt):
    fn = L.lib().ph_debug_conv3x3_route
    out, got = L.ConvRouteOut(), []
    for c in cases:
        rc = fn(C.byref(L.ConvRouteCase(**dict(c, ptr_salt=salt))), n_cu, C.byref(out))
        assert rc == 0, (rc, c)
        got.append([out.kernel, out.kv, out.ksplit, out.props])
    return got


def test_route_entry_is_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "posehip.h")).read()
    assert "int ph_debug_conv3x3_route(const ph_conv_route_case* c, int32_t n_cu, ph_conv_route_out* out);" in header
    fields = re.search(r"typedef struct ph_conv_route_case \{(.*?)\} ph_conv_route_case;", header, re.S).group(1)
    names = [n.strip() for decl in fields.split(";") if decl.strip() for n in decl.split(None, 1)[1].split(",")]
    assert names == [n for n, _ in L.ConvRouteCase._fields_] == list(R.FIELDS) + ["split_scratch_bytes"]
    assert L.lib().ph_conv_route_case_size() == C.sizeof(L.ConvRouteCase)
    assert [getattr(L, "KV_" + k) for k in ("DIRECT", "WINO1D", "WINO2D", "W16", "C16", "WINO4", "WINO2D_KS", "SMALLMAP")] == [1, 2, 3, 4, 5, 7, 10, 12]


def test_golden_belongs_to_the_case_table(golden, cases):
    assert golden["n_cases"] == len(cases) == len(golden["routes"]) and golden["n_cu"] == 256
    assert golden["cases_sha256"] == hashlib.sha256(json.dumps(cases, sort_keys=True).encode()).hexdigest()


def test_golden_covers_every_kernel_and_split_form(golden, cases):
    """Conditions on the record, not measurements: each kernel in at least ten cases under default options -- the register-staged kernel, which no layer reaches under default
    options (conv_dma = 1, conv_dma32 = 1), under the two options that select it --, each split-K form in at least ten, a split refused for a too-small scratch at least once."""
    routes = golden["routes"]
    default = Counter(r[0] for c, r in zip(cases, routes) if all(c[k] == v for k, v in R.DEFAULT_OPTIONS.items()))
    for k in range(8):
        if k != R.K_REGSTAGED:
            assert default[k] >= 10, (R.KERNEL_NAMES[k], default[k])
    assert sum(1 for c, r in zip(cases, routes) if r[0] == R.K_REGSTAGED and (c["use_dma"] == 0 or c["dma32"] == 0)) >= 10
    assert not any(r[0] == R.K_REGSTAGED for c, r in zip(cases, routes) if c["use_dma"] and c["dma32"])
    for k in (R.K_WINO2D, R.K_WINO4):
        assert sum(1 for r in routes if r[0] == k and r[2] > 1) >= 10, R.KERNEL_NAMES[k]
    key = lambda c: tuple(sorted((k, v) for k, v in c.items() if k != "split_scratch_bytes"))  # noqa: E731
    big = {key(c): r for c, r in zip(cases, routes) if c["split_scratch_bytes"] == R.SCRATCH_BIG}
    assert any(c["split_scratch_bytes"] == R.SCRATCH_SMALL and r[2] == 1 and r[0] == big[key(c)][0] and big[key(c)][2] > 1 for c, r in zip(cases, routes) if key(c) in big)
    assert all((r[1] == L.KV_WINO2D_KS) == (r[0] == R.K_WINO2D and r[2] > 1) for r in routes)


def test_every_case_of_the_golden_is_reproduced(golden, cases):
    got = _routes(cases, golden["n_cu"], 0)
    wrong = [(i, cases[i], golden["routes"][i], got[i]) for i in range(len(cases)) if got[i] != golden["routes"][i]]
    assert not wrong, f"{len(wrong)} of {len(cases)} routes differ from the record; first: {wrong[0]}"


def test_route_is_independent_of_pointer_values(golden, cases):
    assert _routes(cases, golden["n_cu"], 1) == _routes(cases, golden["n_cu"], 12345) == golden["routes"]
