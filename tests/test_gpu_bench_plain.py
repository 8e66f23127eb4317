"""GPU: a plain `bench.py --gpus 1` run -- the timed steps and the result line, nothing else -- and what --dump-outputs writes:
z of the last timed step, checked against the oracle on the matrix and x rebuilt from the seeds bench.py uses."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_line_and_outputs(gpu, tmp_path):
    import torch
    import oracle_api as O
    from spgpu_amd import synth
    rows, steps = 200_000, 5
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "2", "--rows", str(rows),
           "--dump-outputs", str(tmp_path)]
    run = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    lines = [ln for ln in run.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, run.stdout[-2000:]
    out = json.loads(lines[0])
    assert out["steps"] == steps and out["warmup"] == 2 and out["ms_per_step"] > 0 and out["value"] > 0
    assert out["unit"] == "GFLOP/s" and out["higher_is_better"] is True and out["dtype"] == "f64" and "SpMV" in out["metric"]
    assert out["config"]["rows"] == rows
    for extra in ("parity", "variants", "configs", "target", "spmm_1gpu", "device"):
        assert extra not in out, extra
    assert sorted(os.listdir(tmp_path)) == ["z.npy"]
    z = np.load(tmp_path / "z.npy")
    assert z.dtype == np.float64 and z.shape == (rows,)
    h = synth.hell_uniform_on_device(rows, 32, "banded", "D", 32, seed=1, device="cuda:0")
    x = synth.device_vector(h["cols"], "D", 3, "cuda:0")
    torch.cuda.synchronize()
    xs = x.cpu().numpy()
    for first in (0, rows - 2048):
        want = O.default_spmv(synth.hell_rows_to_host(h, first, 2048), xs, None, 1.0, 0.0)
        assert z[first:first + 2048].tobytes() == want.tobytes(), first
