"""GPU: tools/sweep_amd.bin, the plain-C caller of include/spgpu/ext/sweep_device.h: the 7-point Laplacian of an 8^3 grid is coloured
and planned on the device, one symmetric sweep on A itself is compared bit for bit with the tool's own plain-C restatement, and
symmetric sweeps go on until the residual call reports the bound of gs_amd (PASSED, exit status 0).  The counts it prints are
numpy's (spgpu_amd.formats) and the launch rule's."""
import re

import pytest

import colour_cases as K
from test_gpu_c_harness import _run

pytestmark = pytest.mark.gpu


def test_sweep_tool_passes_its_own_byte_check_and_converges():
    n = 8
    out = _run("sweep_amd", n)                                                # asserts exit status 0
    rows, colours, rounds = K.TABLE["grid7_8"][:3]
    lines = out.splitlines()
    assert lines[-1] == "PASSED", out
    # 512 rows in 6 colours: every colour is narrow, so a symmetric sweep is one launch forwards and one backwards
    assert f"({rows} rows, {7 * rows - 6 * n * n} nnz): {colours} colours in {rounds} rounds, 2 launches a sweep" in lines[0], out
    assert "first sweep equal to the host's bit for bit" in lines[0], out
    sweeps = int(re.match(r"(\d+) sweeps", lines[1]).group(1))
    assert "(converged)" in lines[1] and 1 < sweeps < 2000, out
    device = float(re.search(r"= ([0-9.e+-]+) on the device", lines[1]).group(1))
    assert device <= 1e-8, out
