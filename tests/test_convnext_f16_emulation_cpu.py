"""tools/convnext_f16_emulation.py (the CPU study that chose the fp16 ConvNeXt path's residual storage) is itself pinned: with nothing
rounded it is ``oracle.cpu_ref.model_forward``; its fp16 modes stay inside the fp16 bar on the configuration the GPU tests run."""
import importlib.util
import os

import torch

from oracle import cpu_ref as O

_spec = importlib.util.spec_from_file_location("convnext_f16_emulation", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "convnext_f16_emulation.py"))
E = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(E)


def _setup():
    label, bb, heads, mt, img, seed, ls = E.cases()[0]
    assert label.startswith("16-128")
    sd = O.init_state_convnext(bb, heads, mt, seed=seed, head_scale=1.0, layer_scale=ls, randomize_affine=True)
    return bb, heads, mt, img, sd


def test_fp32_mode_is_the_oracle():
    bb, heads, mt, img, sd = _setup()
    collect_ref, collect = {}, {}
    ref = O.model_forward(sd, bb, heads, mt, img, collect=collect_ref, backbone="convnext")
    got = E.forward(sd, bb, heads, mt, img, "fp32", collect=collect)
    assert set(got) == set(ref)
    for k, t in ref.items():
        assert (got[k] - t).abs().max().item() <= 1e-5 * max(1.0, t.abs().max().item()), k
    assert set(collect) == set(collect_ref)
    for k, t in collect_ref.items():
        assert (collect[k] - t).abs().max().item() <= 1e-5 * max(1.0, t.abs().max().item()), k


def test_fp16_storage_modes_round_and_stay_inside_the_bar():
    bb, heads, mt, img, sd = _setup()
    ref = O.model_forward(sd, bb, heads, mt, img, backbone="convnext")
    for mode in ("f16", "f16_res32"):
        got = E.forward(sd, bb, heads, mt, img, mode)
        for k, t in ref.items():
            err = (got[k] - t).abs().max().item() / max(1.0, t.abs().max().item())
            assert 0.0 < err <= 5e-3, (mode, k, err)  # rounded somewhere, and with room under the reference's fp16 bar


def test_cases_cover_the_gpu_configurations_and_tiny():
    labels = [c[0] for c in E.cases()]
    assert len(labels) == 5 and labels[-1].startswith("tiny")
    assert torch.is_tensor(E.cases()[-1][4]) and tuple(E.cases()[-1][4].shape) == (1, 3, 96, 96)
