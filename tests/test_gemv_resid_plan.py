"""When a decode norm edge takes the producer-epilogue form (gemv_resid_edge, fastllm_amd/csrc/gemv_geometry.h): the predicate is
plain C++ next to the grid rule, so it is compiled here with the host compiler alone, as tests/test_gemv_geometry.py does."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fastllm_amd", "csrc")

CUS, R = 256, 2


def case(N, K, Nc, fb=0, fw=0, bf16=1, one_shard=1, compute=1, cus=CUS, r=R):
    return [N, K, Nc, r, cus, fb, fw, bf16, one_shard, compute]


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("gemv_resid_plan") / "gemv_resid_plan")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I" + CSRC, os.path.join(ROOT, "tests", "host", "gemv_resid_plan_main.cc"), "-o", exe])

    def run(args):
        out = subprocess.run([exe] + [str(v) for v in args], capture_output=True, text=True, check=True).stdout
        return [tuple(int(x) for x in line.split()) for line in out.splitlines()]
    return run


def test_the_edges_of_mistral_7b_and_tinyllama_fit(plan):
    # Mistral-7B: o_proj -> gate/up, down_proj -> QKV, down_proj -> lm_head; 2048 row groups on 256 x 8 waves, 16 rows per workgroup
    got = plan(case(4096, 4096, 28672) + case(4096, 14336, 6144) + case(4096, 14336, 32000))
    assert got == [(1, 256, 8)] * 3, got
    # TinyLlama-1.1B: 256 x 4 waves, 8 rows per workgroup
    got = plan(case(2048, 2048, 11264) + case(2048, 5632, 2560) + case(2048, 5632, 32000))
    assert got == [(1, 256, 4)] * 3, got
    # the smallest shapes of tests/test_gpu_gemv_resid.py: one and two workgroups of four waves
    assert plan(case(8, 64, 64) + case(16, 1024, 64)) == [(1, 1, 4), (1, 2, 4)]


def test_what_keeps_the_norm_prologue(plan):
    # Qwen2-7B's h = 3584: 1792 row groups on 256 x 7 waves, 14 rows per workgroup -- not whole chunks of 8
    assert plan(case(3584, 3584, 37888)) == [(0, 256, 7)]
    # a forced grid (either half of the knob), fp32, a tensor-parallel shard, FP8 weights
    for kw in (dict(fb=304, fw=6), dict(fb=304), dict(fw=6), dict(bf16=0), dict(one_shard=0), dict(compute=0)):
        assert plan(case(4096, 4096, 28672, **kw))[0][0] == 0, kw
    # a consumer whose workgroups have fewer threads than the vector has chunks: 4096 / 8 = 512 chunks on the 4 x 64 threads of a
    # matrix smaller than the chip
    assert plan(case(4096, 4096, 512))[0][0] == 0
    assert plan(case(2048, 2048, 512))[0][0] == 1
    # four rows per group: 2048 rows are 512 groups on 128 x 4 waves, 16 rows per workgroup; at h = 4096 the gate/up consumer's 7168
    # groups go on 256 x 7 waves, whose 448 threads are fewer than the 512 chunks
    assert plan(case(2048, 2048, 11264, r=4)) == [(1, 128, 4)]
    assert plan(case(4096, 4096, 28672, r=4)) == [(0, 256, 4)]


@pytest.mark.parametrize("cus", [256, 304, 64])
def test_every_yes_covers_n_exactly(plan, cus):
    """N = 8 ... 8192 in steps of 8: a yes means blocks x waves x R == N (exact cover, one row group per wave) and waves x R a multiple
    of 8 (a workgroup's rows are whole chunks of the consumer's K)"""
    rows = plan(["sweep", 4096, 32000, R, cus])
    assert len(rows) == 1024
    yes = 0
    for i, (ok, blocks, waves) in enumerate(rows):
        N = 8 * (i + 1)
        if not ok:
            continue
        yes += 1
        assert blocks * waves * R == N, (N, blocks, waves)
        assert (waves * R) % 8 == 0, (N, blocks, waves)
        assert N // R <= blocks * waves, (N, blocks, waves)
        assert 4 <= waves <= 12
    assert yes > 0
    if cus == 256:
        by_n = {8 * (i + 1): r for i, r in enumerate(rows)}
        assert by_n[4096][0] == 1 and by_n[2048][0] == 1 and by_n[3584][0] == 0
