"""conv3x3_wino4_kernel stores, bit for bit, what it stored before the select and address instructions left its K loop ("Non-arithmetic vector
instructions"): the six launches of tests/_wino4_bits.py against the fixtures tools/gen_wino4_bits_golden.py wrote from the parent build (tests/golden/wino4_bits/).
One process, one launch per case."""
import numpy as np
import pytest
import torch

from tests import _wino4_bits as B

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", B.CASES, ids=lambda c: c.name)
def test_bits_are_the_parents(case):
    want = np.load(B.golden_path(case))
    got = B.run(case, torch.cuda.get_device_properties(0).multi_processor_count)
    assert got.dtype == np.float32 and got.shape == want.shape, (case.name, got.shape, want.shape)
    diff = got.view(np.uint32) != want.view(np.uint32)
    print(f"{case.name}: {int(diff.sum())} of {diff.size} elements differ")
    assert np.array_equal(got, want), (case.name, int(diff.sum()), "elements differ; largest difference", float(np.abs(got - want).max()))
