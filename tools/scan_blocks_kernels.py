"""Developer tool: the kernels of olap_store_blocks_report beside the kernels they are measured against, in one process.

  rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python3 tools/scan_blocks_kernels.py 1000000

splits the run by kernel.  One Float32 store (default 0) per shape, each call repeated REPS times:
  rows        [n/10000, 100, 100] scanned {1}: the innermost dimension kept (blocks_rows_kernel, 16-byte lanes)
  transpose   [sqrt(n), sqrt(n)]  scanned {1}: the innermost dimension scanned (blocks_transpose_kernel)
  get_data_f64 of the same store (to_f64_kernel: the conversion alone, no regrouping)
  reorder [sqrt(n), sqrt(n)] by [1, 0] (the two-axis transpose of 4-byte cells: the regrouping alone, no conversion)
The kernels' algorithmic bytes: 4 read + 8 written per cell (blocks, to_f64), 4 + 4 (reorder).
"""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
from conftest import load_package  # noqa: E402

pkg = load_package()
hipstore = sys.modules[pkg.HipStore.__module__]
REPS = 5


def store(n, seed):
    rng = np.random.default_rng(seed)
    vals = rng.integers(-50, 50, size=n).astype(np.float32)  # zeros are unset
    s = pkg.HipStore(n, "float32", 0.0)
    s.set_data(vals)
    return s


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 1000000
    side = int(math.isqrt(n))
    rows_lens, square = [n // 10000, 100, 100], [side, side]
    a, b = store(n // 10000 * 10000, 1), store(side * side, 2)
    for _ in range(REPS):
        out, launches = hipstore.blocks_report([a], rows_lens, [0, 1, 0])
        assert launches == 1
    want = a.get_data_f64().reshape(rows_lens).transpose(1, 0, 2).reshape(out.shape[1:])
    assert np.array_equal(out[0], want)
    for _ in range(REPS):
        out, launches = hipstore.blocks_report([b], square, [0, 1])
    assert np.array_equal(out[0], b.get_data_f64().reshape(square).T)
    for _ in range(REPS):
        b.get_data_f64()
        b.reorder(square, [1, 0])
    print("cells %d: rows %s scanned {1}; transpose %s scanned {1}; %d repetitions each" % (n, rows_lens, square, REPS))


main()
