"""The token map of the window-attention kernels (csrc/window_attn.h) without a GPU: ``ph_debug_window_tokens`` fills it on the host from the functions the five kernels
call, and it is held here to the reference's own construction -- pad, ``torch.roll``, window partition -- and to the band mask as torchvision / HuggingFace build theirs
from region labels.  The cases are the smallest at which each branch of the geometry is live."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from sleap_nn_amd import _lib as L
from sleap_nn_amd import build
from tests import swinv2_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (w, sh, sw, B, H, W, code_bits)
CASES = [
    (2, 1, 1, 2, 5, 7, 4),      # smallest window
    (2, 1, 1, 2, 5, 7, 5),
    (7, 3, 3, 2, 9, 15, 4),     # padding on both axes
    (7, 0, 3, 1, 7, 15, 4),     # mixed shift: rows off, columns on
    (8, 4, 4, 2, 8, 16, 4),     # one window covers H, rolled and masked anyway (the HuggingFace rule)
    (8, 7, 7, 1, 13, 9, 4),     # shift at its maximum, w - 1
    (9, 4, 4, 2, 10, 19, 5),    # key-tiled range
    (16, 8, 8, 1, 20, 36, 5),
    (24, 12, 12, 1, 30, 25, 5),
    (4, 0, 0, 1, 4, 4, 4),      # one window, no shift: no band anywhere
]


def tokens(w, sh, sw, B, H, W, bits, capacity=None):
    """-> (return code, pix, code) of ph_debug_window_tokens, the arrays as (windows, N)."""
    n = B * -(-H // w) * -(-W // w) * w * w
    pix = np.full(n if capacity is None else max(capacity, 1), -7, dtype=np.int32)
    code = np.full_like(pix, -7)
    rc = L.lib().ph_debug_window_tokens(B, H, W, w, sh, sw, bits, C.c_void_p(pix.ctypes.data), C.c_void_p(code.ctypes.data), pix.size if capacity is None else capacity)
    return rc, pix.reshape(-1, w * w) if capacity is None else pix, code.reshape(-1, w * w) if capacity is None else code


def axis_labels(P, w, s):
    """Region labels of one padded axis, as the slices (0, -w), (-w, -s), (-s, None) of torchvision / HuggingFace number them; an unshifted axis is one region."""
    i = torch.arange(P)
    return (i >= P - w).long() + (i >= P - s).long() if s > 0 else torch.zeros(P, dtype=torch.long)


def reference(w, sh, sw, B, H, W):
    """-> (pix (windows, N) from pad + roll + partition of an index image, masked (windows, N, N) bool from the region labels)."""
    pH, pW = -(-H // w) * w, -(-W // w) * w
    img = torch.arange(B * H * W, dtype=torch.int64).view(B, H, W)
    img = F.pad(img, (0, pW - W, 0, pH - H), value=-1)
    img = torch.roll(img, shifts=(-sh, -sw), dims=(1, 2))
    pix = R.partition(img.unsqueeze(-1), w).view(-1, w * w)
    lab = (axis_labels(pH, w, sh)[:, None] * 3 + axis_labels(pW, w, sw)[None, :]).view(1, pH, pW, 1)
    lw = R.partition(lab, w).view(-1, w * w)  # (windows of one sample, N)
    masked = (lw.unsqueeze(1) != lw.unsqueeze(2)).repeat(B, 1, 1)
    return pix, masked


@pytest.mark.parametrize("case", CASES, ids=["w%d_s%d_%d_b%d_%dx%d_bits%d" % c for c in CASES])
def test_token_map_is_pad_roll_partition_and_bands_are_the_reference_mask(case):
    w, sh, sw, B, H, W, bits = case
    rc, pix, code = tokens(*case)
    assert rc == 0, L.lib().ph_last_error().decode()
    want_pix, want_masked = reference(w, sh, sw, B, H, W)
    assert pix.shape == tuple(want_pix.shape) and np.array_equal(pix, want_pix.numpy())
    field = (1 << bits) - 1
    t = np.arange(w * w)
    assert np.array_equal(code & field, np.broadcast_to(t // w, code.shape)) and np.array_equal((code >> bits) & field, np.broadcast_to(t % w, code.shape))
    band = code >> (2 * bits)
    assert band.min() >= 0 and band.max() <= 3
    assert np.array_equal(band[:, :, None] != band[:, None, :], want_masked.numpy())
    if sh == sw:  # the HuggingFace mask of an equally shifted layer, as the kernel tests' reference builds it
        m = R.shift_mask(-(-H // w) * w, -(-W // w) * w, w, sh, torch.float32)
        hf = torch.zeros_like(want_masked) if m is None else (m != 0).repeat(B, 1, 1)
        assert torch.equal(hf, want_masked)
    if sh == 0 and sw == 0:
        assert not want_masked.any() and not band.any()
    real = np.sort(pix[pix >= 0])
    assert np.array_equal(real, np.arange(B * H * W))  # every real pixel exactly once over all windows


def test_refusals():
    lib = L.lib()
    err = lambda: lib.ph_last_error().decode()  # noqa: E731
    assert tokens(1, 0, 0, 1, 4, 4, 4)[0] != 0 and "window_size" in err()
    assert tokens(25, 0, 0, 1, 30, 30, 5)[0] != 0 and "window_size" in err()
    assert tokens(4, 4, 0, 1, 9, 9, 4)[0] != 0 and "shift" in err()
    assert tokens(4, 0, 4, 1, 9, 9, 4)[0] != 0 and "shift" in err()
    assert tokens(17, 0, 0, 1, 17, 17, 4)[0] != 0 and "code_bits" in err()
    assert tokens(17, 0, 0, 1, 17, 17, 5)[0] == 0
    rc, pix, code = tokens(7, 3, 3, 2, 9, 15, 4, capacity=2 * 2 * 3 * 49 - 1)
    assert rc != 0 and "capacity" in err() and (pix == -7).all() and (code == -7).all()  # nothing written


def test_abi_and_build():
    with open(os.path.join(ROOT, "include", "posehip.h")) as f:
        header = f.read()
    assert int(re.search(r"^#define\s+PH_VERSION\s+(\d+)", header, re.M).group(1)) >= 134
    assert "int ph_debug_window_tokens(" in header and "ph_debug_window_tokens" in L.SIGNATURES
    assert "window_attn.h" in build.HEADERS and os.path.exists(os.path.join(build.CSRC, "window_attn.h"))
