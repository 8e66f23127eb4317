"""GPU: tools/pcg_amd.c -- Jacobi-preconditioned CG written against the C ABI (include/spgpu/ext/precond.h) on A = S L S, a 5-point
Laplacian whose diagonal is spread over three orders of magnitude.  The inverted diagonal from spgpuDhellDiag equals the host's, the
iteration captured as one graph of 5 kernels repeats the eager run with host scalars bit for bit, PCG converges where plain CG
does not.  (numpy on the CPU, 32 x 32 grid, three seeds: Jacobi-PCG reaches 1e-8 in about 91 iterations; plain CG is at 2.4e-4 ...
3.0e-4 after 200 and needs 8 600 - 9 700.)"""
import os
import re
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_pcg_converges_and_the_graph_repeats_the_eager_run():
    exe = os.path.join(ROOT, "tools", "pcg_amd.bin")
    assert os.path.exists(exe), f"{exe} missing: run `make tools`"
    out = subprocess.run([exe, "32", "200", "1e-8"], capture_output=True, text=True, timeout=120)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "PASSED" in out.stdout and "bit-identical to the eager run" in out.stdout and "DIFFERS" not in out.stdout
    assert "dinv from spgpuDhellDiag: equal to" in out.stdout
    pcg = re.search(r"PCG: (\d+) iterations, .* relative residual (\S+) \(converged\)", out.stdout)
    assert pcg and int(pcg.group(1)) <= 200 and float(pcg.group(2)) <= 1e-8, out.stdout
    plain = re.search(r"plain CG: relative residual (\S+) after 200 iterations", out.stdout)
    assert plain and float(plain.group(1)) > 1e-6, out.stdout
