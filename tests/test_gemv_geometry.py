"""The grid rule of the decode weight streams (fastllm_amd/csrc/gemv_geometry.h): one header, no HIP in it, shared by the
bf16 / fp32 stream (under the fl_tune grid) and the FP8 stream (without it)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fastllm_amd", "csrc")

CUS, R = 256, 2
# N x K -> (workgroups, waves per workgroup) at 256 CUs, two rows per group, bf16 activations in LDS (2 K bytes), no forced grid:
# the decode projections of Mistral-7B, Qwen2-7B and TinyLlama-1.1B, and a matrix smaller than the chip
TABLE = [
    (6144, 4096, 256, 12), (4096, 4096, 256, 8), (28672, 4096, 256, 8), (4096, 14336, 256, 8), (32000, 4096, 256, 9),
    (4608, 3584, 256, 9), (37888, 3584, 256, 5), (3584, 18944, 256, 7), (152064, 3584, 256, 11),
    (2560, 2048, 256, 5), (11264, 2048, 256, 11), (2048, 5632, 256, 4),
    (64, 64, 8, 4),
]


def case(N, K, fb=0, fw=0):
    return [(N + R - 1) // R, (2 * K + 15) & ~15, CUS, fb, fw]


@pytest.fixture(scope="module")
def geometry(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("gemv_geometry") / "gemv_geometry")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I" + CSRC, os.path.join(ROOT, "tests", "host", "gemv_geometry_main.cc"), "-o", exe])

    def run(cases):
        out = subprocess.run([exe] + [str(v) for c in cases for v in c], capture_output=True, text=True, check=True).stdout
        return [tuple(int(x) for x in line.split()) for line in out.splitlines()]
    return run


def test_automatic_grid_of_the_decode_projections(geometry):
    got = geometry([case(N, K) for N, K, _, _ in TABLE])
    assert got == [(b, w) for _, _, b, w in TABLE], list(zip(TABLE, got))


def test_forced_grid_is_returned_as_given(geometry):
    assert geometry([case(32000, 4096, 304, 6), case(64, 64, 3, 12)]) == [(304, 6), (3, 12)]


def test_rule_without_the_knob(geometry):
    # (0, 0) -- what the FP8 stream passes -- is the automatic rule; so is a knob of which only one half is set
    auto = geometry([case(32000, 4096)])
    assert auto == [(256, 9)]
    assert geometry([case(32000, 4096, 0, 0), case(32000, 4096, 304, 0), case(32000, 4096, 0, 6)]) == auto * 3
