"""The K loop of conv3x3_wino4_kernel keeps the vector-instruction count it was brought to ("Non-arithmetic vector instructions"): on the fp32 matrix
pipe every vector instruction beside the MFMAs adds its cycles, whatever it computes, and a select or an address rebuilt per quarter shows in no functional test.

The file is compiled to gfx950 assembly (no GPU needed) and the loop bodies of the two forward instantiations are read: a body is a basic block with one barrier and at
least 12 MFMAs (the part of a quarter behind its halo loads).  Per body the vector instructions that are not MFMAs are counted -- instruction classes only -- and held to
what the change reached; the parent's bodies held 32 (xi 0 / 5 waves) and 57 (xi-pair waves) at full resolution, 50 and 93 with the folded bilinear, five of each a
`v_cndmask_b32` between two values fixed for the whole tile (the weight loads' "beyond the slice" offset: now a scalar choice of the buffer descriptor)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL_RES = "_ZN2ph20conv3x3_wino4_kernelILb0ELb0EEEvNS_8ConvArgsE"
LOW_RES = "_ZN2ph20conv3x3_wino4_kernelILb1ELb0EEEvNS_8ConvArgsE"


def _hipcc():
    return shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)


@pytest.fixture(scope="module")
def bodies(tmp_path_factory):
    """kernel name -> [(vector instructions, selects)] of its K-loop bodies."""
    hipcc = _hipcc()
    if hipcc is None:
        pytest.skip("hipcc not found")
    src = os.path.join(ROOT, "sleap_nn_amd", "csrc", "wino4_kernels.hip")
    out = tmp_path_factory.mktemp("w4isa") / "wino4.s"
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S", "-I", os.path.join(ROOT, "include"), "-I", os.path.dirname(src), "-o", str(out), src],
                   check=True, capture_output=True, timeout=600)
    found = {}
    for m in re.finditer(r"^(_ZN2ph20conv3x3_wino4_kernel\w+):(.*?)s_endpgm", out.read_text(), re.S | re.M):
        blocks, cur = [], []
        for line in m.group(2).split("\n"):
            s = line.strip()
            if not s or s.startswith((";", "//")):
                continue
            if re.match(r"^[.\w$]+:", s):  # a label starts a block
                blocks.append(cur)
                cur = []
                continue
            if s.startswith("."):
                continue
            cur.append(s.split()[0])
            if s.startswith(("s_cbranch", "s_branch")):  # a branch ends one
                blocks.append(cur)
                cur = []
        blocks.append(cur)
        rows = []
        for b in blocks:
            if sum(i == "s_barrier" for i in b) == 1 and sum(i.startswith("v_mfma") for i in b) >= 12:
                rows.append((sum(i.startswith("v_") and not i.startswith("v_mfma") for i in b), sum(i.startswith("v_cndmask") for i in b)))
        found[m.group(1)] = rows
    return found


def _group_maxima(counts, groups):
    counts = sorted(counts)
    n = len(counts) // groups
    return [max(counts[i * n:(i + 1) * n]) for i in range(groups)]


def test_full_resolution_bodies(bodies):
    """Eight bodies (xi group x "this wave has output channels", two quarters per loop trip): xi 0 / 5 waves, then xi-pair waves.  Parent: 32 / 57."""
    rows = bodies[FULL_RES]
    print(sorted(rows))
    assert len(rows) >= 8 and len(rows) % 2 == 0, rows
    light, pair = _group_maxima([v for v, _ in rows], 2)
    assert light <= 25 and pair <= 49, (light, pair)


def test_folded_bilinear_bodies(bodies):
    """Full-resolution quarters of xi 0 / 5 waves, low-resolution ones, then the same two of xi-pair waves (paired loops and the two single quarters where the transform
    changes).  Parent: 32 / 50 / 57 / 93."""
    rows = bodies[LOW_RES]
    print(sorted(rows))
    assert len(rows) >= 16 and len(rows) % 4 == 0, rows
    maxima = _group_maxima([v for v, _ in rows], 4)
    assert all(got <= bar for got, bar in zip(maxima, (27, 45, 52, 88))), maxima


def test_no_select_in_a_loop_body(bodies):
    """The loop bodies hold no select at all: the five of the parent chose, every quarter, between two values that are fixed for the tile."""
    for name in (FULL_RES, LOW_RES):
        assert bodies[name] and all(sel == 0 for _, sel in bodies[name]), (name, bodies[name])
