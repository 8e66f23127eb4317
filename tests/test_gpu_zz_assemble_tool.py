"""GPU: tools/assemble_amd.bin, the plain-C caller of include/spgpu/ext/assemble_device.h: the element-by-element listing of a P1
Laplacian is assembled, put into HELL and multiplied, assembled again with scaled element matrices through the values-only call and
the refill, and multiplied again; the tool itself compares both products with those of the matrix that keeps every duplicate
(PASSED).  Every number is a small integer, so every sum is exact in fp64 in any order and the tool's checksums equal numpy's
with ==."""
import numpy as np
import pytest

from test_gpu_c_harness import _run

pytestmark = pytest.mark.gpu


def _numpy_checksums(n):
    """The tool's listing, restated: (contributions, entries, {stage: (sum z, sum (i % 7 + 1) z[i], sum of the assembled values)})."""
    local = np.array([[2, -1, -1], [-1, 1, 0], [-1, 0, 1]], np.float64)
    e = np.arange(2 * n * n)
    cell = e // 2
    i, j = cell % n, cell // n
    lower = np.stack((j * (n + 1) + i, j * (n + 1) + i + 1, (j + 1) * (n + 1) + i), axis=1)
    upper = np.stack(((j + 1) * (n + 1) + i + 1, (j + 1) * (n + 1) + i, j * (n + 1) + i + 1), axis=1)
    node = np.where((e % 2 == 0)[:, None], lower, upper)
    rows = np.repeat(node, 3, axis=1).reshape(-1)                 # a outer, b inner
    cols = np.tile(node, (1, 3)).reshape(-1)
    v1 = np.tile(local.reshape(-1), e.size)
    v2 = v1 * np.repeat(e % 5 + 1, 9)
    size = (n + 1) * (n + 1)
    x = np.arange(size) % 13 + 1.0
    weights = np.arange(size) % 7 + 1.0
    out = {}
    for stage, v in (("built", v1), ("scaled", v2)):
        z = np.bincount(rows, weights=v * x[cols], minlength=size)
        out[stage] = (float(z.sum()), float((weights * z).sum()), float(v.sum()))
    return rows.size, np.unique(rows * size + cols).size, out


def test_assemble_tool_checksums_equal_numpy():
    n = 40
    out = _run("assemble_amd", n)
    nnz, entries, want = _numpy_checksums(n)
    lines = out.splitlines()
    assert f"{nnz} contributions, {entries} entries" in lines[0] and lines[-1] == "PASSED", out
    seen = {}
    for line in lines[1:-1]:
        head, numbers = line.split(":")
        seen[head] = tuple(float(t) for t in numbers.split())
    assert sorted(seen) == sorted(want), out
    for stage, got in seen.items():
        assert got == want[stage], (stage, got, want[stage])
    assert want["built"] != want["scaled"] and nnz > 5 * entries // 2
