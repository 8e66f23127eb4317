"""GPU: tools/gs_amd.bin, the plain-C caller of include/spgpu/ext/trsv_device.h, run once: on a 5-point Laplacian one forward and
one backward solve must equal a substitution in plain C bit for bit, and CG preconditioned by symmetric Gauss-Seidel -- two
triangular solves from the matrix's own arrays and a diagonal scaling per iteration -- must converge in fewer iterations than plain
CG on the same system to the same relative residual.  The tool itself decides (PASSED, exit status 0); the test reads the two
iteration counts and the level counts off its output."""
import re

import pytest

from test_gpu_c_harness import _run

pytestmark = pytest.mark.gpu


def test_gauss_seidel_tool_matches_the_substitution_and_beats_plain_cg():
    g = 48
    out = _run("gs_amd", g)                                                 # _run expects exit status 0, under a time limit
    lines = out.splitlines()
    assert lines[-1] == "PASSED", out
    assert f"{2 * g - 1} levels below the diagonal, {2 * g - 1} above" in lines[0], out
    assert "forward solve: equal to the substitution in C (0 of" in out and "backward solve: equal to the substitution in C (0 of" in out
    pcg = int(re.search(r"SGS-PCG: (\d+) iterations", out).group(1))
    cg = int(re.search(r"plain CG: (\d+) iterations", out).group(1))
    assert "(converged)" in out and 0 < pcg < cg, out
