"""GPU: tools/multicolour_amd.bin, the plain-C caller of include/spgpu/ext/colour_device.h: the 7-point Laplacian of an 8^3 grid is
coloured, ordered and permuted on the device, the tool compares B with its own plain-C restatement of P A P^T, counts the levels of
both orders with the Plans of the triangular solve, and runs CG preconditioned by symmetric Gauss-Seidel on both (PASSED, exit
status 0).  The counts it prints are numpy's (spgpu_amd.formats)."""
import re

import pytest

import colour_cases as K
from test_gpu_c_harness import _run

pytestmark = pytest.mark.gpu


def test_multicolour_tool_passes_and_prints_numpys_counts():
    n = 8
    out = _run("multicolour_amd", n)                                          # asserts exit status 0
    rows, colours, rounds, natural, coloured = K.TABLE["grid7_8"]
    lines = out.splitlines()
    assert lines[-1] == "PASSED", out
    assert f"({rows} rows, {7 * rows - 6 * n * n} nnz): {colours} colours in {rounds} rounds" in lines[0] and "B equal to P A P^T" in lines[0], out
    assert lines[1] == (f"levels below / above the diagonal: natural order {natural} / {natural}, "
                        f"multicolour order {coloured} / {coloured}"), out
    iterations = [int(re.search(r": +(\d+) iterations", line).group(1)) for line in lines[2:4]]
    assert all("(converged)" in line for line in lines[2:4]) and all(1 <= it < 2000 for it in iterations), out
