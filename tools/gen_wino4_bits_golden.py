"""Write the bitwise fixtures of tests/test_gpu_wino4_bits.py: python tools/gen_wino4_bits_golden.py [--out DIR]

Run on an MI355X with a build of the commit whose results are to be held (the fixtures in the tree come from the parent of the change that took the non-arithmetic
vector instructions out of the F(4x4,3x3) K loop).  One .npy per case of tests/_wino4_bits.py, float32, under 1 MB in all."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from tests import _wino4_bits as B  # noqa: E402


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=B.GOLDEN_DIR)
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    total = 0
    for case in B.CASES:
        a = B.run(case, n_cu)
        again = B.run(case, n_cu)
        assert a.dtype == np.float32 and np.isfinite(a).all(), (case.name, "an element is not finite")
        assert np.array_equal(a, again), (case.name, "two launches of one case differ")
        path = os.path.join(args.out, os.path.basename(B.golden_path(case)))
        np.save(path, a)
        total += os.path.getsize(path)
        print(f"{case.name}: {a.shape} -> {path} ({os.path.getsize(path)} bytes)")
    assert total < 1_000_000, total
    print(f"{len(B.CASES)} files, {total} bytes")
    return 0


if __name__ == "__main__":
    sys.exit(main())
