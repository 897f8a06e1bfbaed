"""Host-side pieces of Swin training: the C ABI declaration, the stochastic-depth schedule and the drawn branch scales."""
import os
import re

import pytest
import torch

from sleap_nn_amd import _lib as L
from sleap_nn_amd.architectures.swint import ARCH_TYPES, draw_branch_scales, stochastic_depth_probs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_branch_scales_and_version():
    header = open(os.path.join(ROOT, "include", "posehip.h")).read()
    assert int(re.search(r"^#define\s+PH_VERSION\s+(\d+)", header, re.M).group(1)) >= 121
    m = re.search(r"int\s+ph_model_set_branch_scales\s*\(([^)]*)\)", header)
    assert m and len(m.group(1).split(",")) == 4
    assert len(L.SIGNATURES["ph_model_set_branch_scales"][1]) == 4
    assert re.search(r"^#define\s+PH_KV_WINDOW_ATTN_BWD\s+%d\b" % L.SWIN_KV_WINDOW_ATTN_BWD, header, re.M)
    assert "ph_model_last_backward_kernels" in L.SIGNATURES


@pytest.mark.parametrize("name", ["tiny", "small", "base"])
def test_stochastic_depth_schedule_is_the_references(name):
    """swint.py:110-137: block k of all stages in order is dropped with stochastic_depth_prob * k / (total_blocks - 1), 0.1 by default."""
    depths = ARCH_TYPES[name]["depths"]
    total = sum(depths)
    want, k = [], 0
    for d in depths:
        for _ in range(d):
            want.append(0.1 * float(k) / (total - 1))
            k += 1
    got = stochastic_depth_probs(depths)
    assert got == want and got[0] == 0.0 and abs(got[-1] - 0.1) < 1e-12
    assert draw_branch_scales(depths, 3).shape == (2 * total, 3)


def test_drawn_scales_are_zero_or_the_inverse_keep_probability():
    depths, prob, B = [2, 2, 6, 2], 0.4, 64
    s = draw_branch_scales(depths, B, prob, generator=torch.Generator().manual_seed(5))
    p = stochastic_depth_probs(depths, prob)
    assert s.dtype == torch.float32 and s.shape == (2 * sum(depths), B)
    assert bool((s[:2] == 1).all())  # block 0: p = 0
    for k, pk in enumerate(p):
        keep = torch.tensor(1.0 - pk, dtype=torch.float32)
        for row in (s[2 * k], s[2 * k + 1]):
            assert bool(((row == 0) | torch.isclose(row, 1.0 / keep, rtol=1e-6, atol=0.0)).all()), k  # (1e-6: 1 - p_k rounded to fp32 before or after the subtraction)
    assert bool((s == 0).any()) and not torch.equal(s[-1], s[-2])  # the two branches of a block draw independently
    again = draw_branch_scales(depths, B, prob, generator=torch.Generator().manual_seed(5))
    assert torch.equal(s, again)


def test_model_train_names_the_keyword():
    from sleap_nn_amd.architectures.model import Model

    bb = {"model_type": None, "arch": {"embed": 32, "depths": [2, 2, 2, 2], "num_heads": [1, 2, 4, 8]}, "in_channels": 1, "patch_size": 4, "window_size": 7,
          "kernel_size": 3, "filters_rate": 2, "convs_per_block": 2, "up_interpolate": True, "stem_patch_stride": 2, "output_stride": 2, "max_stride": 32}
    heads = {"confmaps": {"part_names": ["a", "b"], "sigma": 2.5, "output_stride": 2}}
    m = Model("swint", bb, heads, "single_instance")
    with pytest.raises(NotImplementedError, match="allow_swint"):
        m.train()
    m.train(True, allow_swint=True)
    assert m.ops is m.unfused_ops and m.residual_branches() == 16
    m.eval()
    assert m.ops is m.fused_ops and m.residual_branches() == 16
