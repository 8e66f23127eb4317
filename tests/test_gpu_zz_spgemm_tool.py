"""GPU: tools/galerkin_amd.bin, the plain-C caller of include/spgpu/ext/spgemm_device.h: a 5-point Laplacian is assembled, P^T comes
out of the transpose and the way back to CSR, R = P^T A and A_c = R P are formed on the device, A_c goes into HELL and is
multiplied; then A gets new coefficients and everything follows through the values-only calls.  The tool itself compares A_c entry
by entry, and the product, with the closed form (PASSED).  Every number is a small integer, so the tool's checksums equal numpy's
with ==."""
import numpy as np
import pytest

from test_gpu_c_harness import _run

pytestmark = pytest.mark.gpu


def _numpy_checksums(n):
    """The closed form, restated: (entries of A, products and entries of R, of A_c, {stage: (sum z, sum (i % 7 + 1) z[i], sum of
    the values of A_c)})."""
    m = n // 2
    coarse = m * m
    I = np.arange(coarse)
    x, y = I % m, I // m
    neighbours = [(x > 0, I - 1), (x < m - 1, I + 1), (y > 0, I - m), (y < m - 1, I + m)]
    v = np.arange(coarse) % 13 + 1.0
    weights = np.arange(coarse) % 7 + 1.0
    links = sum(int(ok.sum()) for ok, _ in neighbours)
    out = {}
    for stage, diagonal in (("built", 4.0), ("recomputed", 6.0)):
        z = (4 * diagonal - 8) * v
        for ok, to in neighbours:
            z[ok] -= 2 * v[to[ok]]
        out[stage] = (float(z.sum()), float((weights * z).sum()), float((4 * diagonal - 8) * coarse - 2 * links))
    fine_entries = n * n + 4 * n * (n - 1)
    # R = P^T A: one product per entry of A; a row of R holds the 4 cells of its aggregate and the 2 cells beyond each side inside
    products_r = fine_entries
    entries_r = 4 * coarse + 2 * links
    # A_c = R P: one product per entry of R (P has one entry per row)
    return fine_entries, products_r, entries_r, entries_r, coarse + links, out


def test_galerkin_tool_checksums_equal_numpy():
    n = 64
    out = _run("galerkin_amd", n)
    fine_entries, products_r, entries_r, products_c, entries_c, want = _numpy_checksums(n)
    lines = out.splitlines()
    assert lines[-1] == "PASSED", out
    assert f"{fine_entries} entries; P: {n * n // 4} aggregates; R = P^T A: {products_r} products, {entries_r} entries; " \
           f"A_c = R P: {products_c} products, {entries_c} entries, longest row 5" in lines[0], out
    seen = {}
    for line in lines[1:-1]:
        head, numbers = line.split(":")
        seen[head] = tuple(float(t) for t in numbers.split())
    assert sorted(seen) == sorted(want), out
    for stage, got in seen.items():
        assert got == want[stage], (stage, got, want[stage])
    assert want["built"] != want["recomputed"]
