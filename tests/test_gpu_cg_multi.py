"""GPU: tools/cg_multi_amd.c -- CG for several right-hand sides at once on pitch multivectors, the consumer of spgpu?hdiaspmmMv
(spgpu/ext/hdia_spmm.h) and of the device-scalar multivector calls (spgpu/ext/device_scalars_mv.h).  One captured graph per block
iteration; the iterates and |r|^2 of every column must repeat the per-column run with the single-vector calls bit for bit."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("count", [8, 3])
def test_block_cg_repeats_the_per_column_run(count):
    """grid 64: n = 4096, 2 workgroups per vector, the cap on workgroups per vector does not bind."""
    exe = os.path.join(ROOT, "tools", "cg_multi_amd.bin")
    assert os.path.exists(exe), f"{exe} missing: run `make tools`"
    out = subprocess.run([exe, "64", "20", str(count)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "PASSED" in out.stdout and "the cap does not bind" in out.stdout
    assert out.stdout.count("bit-identical to the per-column reference") == 2, out.stdout     # the multi and the fused leg
    assert out.stdout.count("gaps untouched") == 3 and "DIFFER" not in out.stdout
