"""GPU: tools/amg_setup_amd.bin, the plain-C caller of include/spgpu/ext/aggregate_device.h: a 5-point Laplacian is assembled, its
strength of connection, aggregates and tentative prolongator T are built on the device, T^T comes out of the transpose and the way
back to CSR, and R = T^T A and A_c = R T are formed on the device.  The tool compares aggregateOf with its own plain-C restatement of
the rounds and checks the sums (PASSED); every number is a small integer, so its summary line equals numpy's restatement
(spgpu_amd.formats) with ==."""
import numpy as np
import pytest

import aggregate_cases as A
from test_gpu_c_harness import _run

pytestmark = pytest.mark.gpu


def test_amg_setup_tool_summary_equals_numpy():
    from spgpu_amd import formats
    n = 16
    out = _run("amg_setup_amd", n)
    ptr, col, vals = A.grid_5pt(n, 1)
    strong, _ = formats.csr_strength(ptr, col, vals, 1, 0.25)
    count, rounds, aggregate_of, sizes = formats.csr_aggregate(ptr, col, strong, 1)
    # the pattern of A_c = T^T A T: aggregates (I, J) joined by a stored entry of A
    row_of = np.repeat(np.arange(n * n), np.diff(ptr))
    coarse_entries = len(set(zip(aggregate_of[row_of].tolist(), aggregate_of[col - 1].tolist())))
    total = float(vals.sum())
    assert total == 4 * n
    lines = out.splitlines()
    assert len(lines) == 1, out
    assert lines[0] == (f"amg_setup n={n} rows={n * n} entries={vals.size} strong={int(strong.sum())} aggregates={count} rounds={rounds} "
                        f"sizes_sum={int(sizes.sum())} coarse_rows={count} coarse_entries={coarse_entries} sum_a={total:.17g} "
                        f"sum_ac={total:.17g} symmetric=1 PASSED"), out
