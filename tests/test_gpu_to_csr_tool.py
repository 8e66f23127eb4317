"""GPU: tools/to_csr_amd.bin, the plain-C caller of include/spgpu/ext/to_csr_device.h: CSR -> HELL -> CSR gives the caller's arrays,
and the HELL arrays of A^T -> CSR give the CSC arrays of A (memcmp in the tool)."""
import pytest

from test_gpu_c_harness import _run

pytestmark = pytest.mark.gpu


def test_to_csr_tool_reports_ok_for_both_legs():
    out = _run("to_csr_amd")
    lines = [line for line in out.splitlines() if line.endswith(("OK", "MISMATCH"))]
    assert len(lines) == 2 and all(line.endswith(": OK") for line in lines), out
    assert lines[0].startswith("HELL -> CSR") and lines[1].startswith("HELL of A^T -> CSR")


def test_to_csr_tool_on_a_wide_matrix():
    out = _run("to_csr_amd", 257, 5000)      # more columns than rows: most rows of A^T are empty
    assert out.count(": OK") == 2 and "MISMATCH" not in out, out
