"""CPU: spgpu_amd/csrc/csr_host.h -- the host rules the device calls on CSR arrays share (the capped grid, the key bits of a count, the
dispatch on the value type) -- executed.  tests/csr_host_cases.cpp is a stand-alone program around that header (g++,
undefined-behaviour sanitizer on); what it answers is compared with the rules as the header's comments state them, restated here."""
import subprocess

import pytest

from spgpu_amd import capi
from spmv_launch_shapes import rules_program

MAX_BLOCKS = 1048576
LLONG_MAX = 2 ** 63 - 1


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return rules_program(tmp_path_factory.mktemp("csr_host"), "csr_host_cases")


def run(program, lines):
    done = subprocess.run([program], input="".join(line + "\n" for line in lines), capture_output=True, text=True)
    assert done.returncode == 0 and "runtime error" not in done.stderr, (done.returncode, done.stderr[-2000:])
    out = [line.split() for line in done.stdout.splitlines()]
    assert len(out) == len(lines) + 1 and out[-1][0] == "constants"
    return out[:-1], int(out[-1][1])


def grid(items, per_block, max_blocks):
    """at least 1 workgroup, at most maxBlocks (> 0) or kCsrMaxBlocks, else one per perBlock items"""
    return max(1, min((items + per_block - 1) // per_block, max_blocks if max_blocks > 0 else MAX_BLOCKS))


def test_the_cap_is_the_one_of_the_other_grid_rules(program):
    _, cap = run(program, [])
    assert cap == MAX_BLOCKS


@pytest.mark.parametrize("per_block", [1, 4, 256])
@pytest.mark.parametrize("max_blocks", [0, 3])
def test_capped_grid(program, per_block, max_blocks):
    cap = max_blocks if max_blocks > 0 else MAX_BLOCKS
    items = [0, 1, per_block, per_block + 1, per_block * cap, per_block * cap + 1, LLONG_MAX // 2 - 7, LLONG_MAX // 2]
    got, _ = run(program, [f"grid {n} {per_block} {max_blocks}" for n in items])
    assert [(kind, int(value)) for kind, value in got] == [("grid", grid(n, per_block, max_blocks)) for n in items]
    assert [int(value) for _, value in got][:2] == [1, 1] and int(got[-1][1]) == cap and int(got[4][1]) == cap == int(got[5][1])
    assert int(got[3][1]) == min(2, cap)


def test_an_addgridfor_call_is_the_one_item_per_block_case(program):
    got, _ = run(program, ["grid -5 1 0", "grid 7 1 0", "grid 7 1 2", f"grid {MAX_BLOCKS + 9} 1 0"])
    assert [int(value) for _, value in got] == [1, 7, 2, MAX_BLOCKS]


def test_bits_for(program):
    counts = [1, 2, 3, 4, 2 ** 31 - 1, 2 ** 31]
    got, _ = run(program, [f"bits {n}" for n in counts])
    for n, (kind, b) in zip(counts, got):
        b = int(b)
        assert kind == "bits" and 2 ** b >= n and (b == 0 or 2 ** (b - 1) < n), n      # the smallest b with 2^b >= n
    assert [int(b) for _, b in got] == [0, 1, 2, 2, 31, 31]


def test_for_value_type(program):
    sizes = {capi.TYPE_FLOAT: (4, 1), capi.TYPE_DOUBLE: (8, 1), capi.TYPE_COMPLEX_FLOAT: (8, 0), capi.TYPE_COMPLEX_DOUBLE: (16, 0)}
    codes = sorted(sizes) + [capi.TYPE_INT, 5, -1]
    got, _ = run(program, [f"type {code}" for code in codes])
    for code, (kind, known, calls, size, real) in zip(codes, got):
        assert kind == "type"
        if code in sizes:
            assert (int(known), int(calls), int(size), int(real)) == (1, 1) + sizes[code], code
            assert int(size) == capi.spgpuSizeOf(code)
        else:
            assert (int(known), int(calls), int(size)) == (0, 0, 0), code
