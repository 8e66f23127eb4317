"""GPU: tools/update_amd.bin, the plain-C caller of include/spgpu/ext/update_device.h: a HELL matrix is built from CSR, multiplied,
refilled, multiplied, partly overwritten through spgpuDhellcsput and multiplied again -- as the rows come and stored in reverse
row order.  Every number involved is a small multiple of 1/8, so every sum is exact in fp64 in any order and the tool's checksums
equal numpy's with ==."""
import numpy as np
import pytest

from test_gpu_c_harness import _run

pytestmark = pytest.mark.gpu


def _numpy_checksums(rows):
    """The tool's matrix, vectors and update list, restated: {stage: (sum z, sum (i % 7 + 1) z[i], sum of the coefficients)}."""
    base = 1
    lengths = (np.arange(rows, dtype=np.int64) * 7) % 23
    ptr = np.concatenate(([0], np.cumsum(lengths)))
    nnz = int(ptr[-1])
    row = np.repeat(np.arange(rows), lengths)
    k = np.arange(nnz) - ptr[row]
    col = row % 11 + 3 * k                                        # 0-based
    e = np.arange(nnz, dtype=np.float64)
    v1 = e * 0.25 + 0.25
    v2 = -(np.arange(nnz) % 1001).astype(np.float64) * 0.5 - 0.75
    v3 = v2.copy()
    third = k % 3 == 0
    v3[third] = (row[third] % 97) * 2.0 + 0.125                   # the two list entries that must be ignored change nothing
    x = (np.arange(rows + 80) % 13) * 0.5 + 1.0
    weights = np.arange(rows) % 7 + 1.0
    out = {}
    for stage, v in (("built", v1), ("refilled", v2), ("csput", v3)):
        z = np.bincount(row, weights=v * x[col], minlength=rows)
        out[stage] = (float(z.sum()), float((weights * z).sum()), float(v.sum()))
    return out, nnz, int(third.sum()) + 2


@pytest.mark.parametrize("rows", [1000, 97])
def test_update_tool_checksums_equal_numpy(rows):
    out = _run("update_amd", rows)
    want, nnz, listed = _numpy_checksums(rows)
    assert f"{nnz} entries, {listed} list entries" in out.splitlines()[0], out
    seen = {}
    for line in out.splitlines()[1:]:
        head, numbers = line.split(":")
        seen[tuple(head.split())] = tuple(float(t) for t in numbers.split())
    assert sorted(seen) == sorted((order, stage) for order in ("natural", "reversed") for stage in want), out
    for (order, stage), got in seen.items():
        assert got == want[stage], (order, stage, got, want[stage])
    assert want["built"] != want["refilled"] != want["csput"]
