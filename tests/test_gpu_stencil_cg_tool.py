"""GPU: tools/cg_hdia_amd.c -- CG and Jacobi-PCG on a 7-point Laplacian kept in HDIA, written against the C ABI
(include/spgpu/ext/hdia_solver.h).  The captured iteration with the fused spgpuDhdiaspmvDotDevice (5 kernels) repeats the one from
spgpuDhdiaspmv + spgpuDdotDevice bit for bit -- the iterate and the last |r|^2 -- and |r|^2 has fallen.  (numpy on the CPU, 32^3
grid, 30 iterations: |r|^2 falls by 8.5e-4 for CG and by 1.8e-6 for Jacobi-PCG on the scaled matrix.)  Named, like
tests/test_gpu_stencil_dot.py, to be collected behind the GPU modules the suite already had."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("mode", [(), ("jacobi",)], ids=["cg", "jacobi"])
def test_the_fused_leg_repeats_the_unfused_one(mode):
    exe = os.path.join(ROOT, "tools", "cg_hdia_amd.bin")
    assert os.path.exists(exe), f"{exe} missing: run `make tools`"
    out = subprocess.run(["timeout", "-k", "10", "120", exe, "32", "30", *mode], capture_output=True, text=True)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "PASSED" in out.stdout and "DIFFERS" not in out.stdout and "has fallen" in out.stdout
    assert ("dinv from spgpuDhdiaDiag: equal to" in out.stdout) == bool(mode)
