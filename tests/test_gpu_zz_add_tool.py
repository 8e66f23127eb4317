"""GPU: tools/timestep_amd.bin, the plain-C caller of include/spgpu/ext/add_device.h: a 5-point stiffness matrix K and a narrower
mass matrix M are assembled separately, C = M + dt K is formed on the device, goes into HELL and is multiplied by the vector of
ones; then K gets new coefficients and dt a new value, and everything follows through the values-only calls.  The tool itself
compares every row sum with the closed form (PASSED, exit status 0).  Every number is a small multiple of 1/4, so the tool's
checksums equal numpy's with ==."""
import numpy as np
import pytest

from test_gpu_c_harness import _run

pytestmark = pytest.mark.gpu


def _numpy_checksums(n):
    """The closed form, restated: (entries of K, of M, {stage: (sum z, sum (i % 7 + 1) z[i], sum of the values of C)})."""
    i = np.arange(n * n)
    x, y = i % n, i // n
    mx = (x > 0).astype(float) + (x < n - 1)
    kx = mx + (y > 0) + (y < n - 1)
    weights = i % 7 + 1.0
    out = {}
    for stage, diagonal, dt in (("built", 4.0, 0.5), ("stepped", 6.0, 0.25)):
        z = 4.0 + mx + dt * (diagonal - kx)
        out[stage] = (float(z.sum()), float((weights * z).sum()), float(z.sum()))
    return n * n + int(kx.sum()), n * n + int(mx.sum()), out


def test_timestep_tool_checksums_equal_numpy():
    n = 64
    out = _run("timestep_amd", n)                                           # _run expects exit status 0, under a time limit
    k_entries, m_entries, want = _numpy_checksums(n)
    lines = out.splitlines()
    assert lines[-1] == "PASSED", out
    assert f"{k_entries} entries; M: {m_entries} entries; C = M + dt K: {k_entries} entries, longest row 5" in lines[0], out
    seen = {}
    for line in lines[1:-1]:
        head, numbers = line.split(":")
        seen[head] = tuple(float(t) for t in numbers.split())
    assert sorted(seen) == sorted(want), out
    for stage, got in seen.items():
        assert got == want[stage], (stage, got, want[stage])
    assert want["built"] != want["stepped"]
