"""The prefill attention plans (fastllm_amd/csrc/attn_prefill_plan.h): which kernel a prompt runs -- 16 or 32 rows per wave -- and its
launch, and the token sub-tiles and key split of a pack.  One header, no HIP in it, compiled here with the host compiler.

The expected table (tests/golden/attn_prefill_plan.txt) is NOT this header's output: it was printed by the selection text of the
commit before the header existed (launch_attn_prefill_mfma, launch_pf32, attn_packed_geometry), copied into a program whose tune()
returns the switch set of the case and whose launches print their template arguments, grid, block, LDS bytes and tag
(profiles/attn_prefill16/README.md).  A line is the case's arguments, " | ", and that output."""
import os
import subprocess

import pytest

from test_gpu_kernel_selection import TS
from test_gpu_packed_attention import PACKS, expected_tt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fastllm_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden", "attn_prefill_plan.txt")

# (H, Hkv, d): Mistral-7B, Qwen2-7B, TinyLlama-1.1B, G = 3, G = 8 -- each also at the other head size
SHAPES = [(H, Hkv, d) for H, Hkv in [(32, 8), (28, 4), (32, 4), (6, 2), (8, 1)] for d in (128, 64)]
LENGTHS = sorted(set(TS + [352, 576, 577, 600, 639, 640, 1536, 2048, 3072, 4096, 4608]))
DEFAULT = dict(pf32_min_t=0, pf32_ks2=-1, pf32_paired=-1, pf_waves=0, pf_stages=2, pf_ksplit=2)      # runtime.hip's table
SETS = [{}] + [{"pf32_ks2": v} for v in (0, 1, 4)] + [{"pf32_paired": v} for v in (0, 1, 2)] + [{"pf_waves": 8}, {"pf_ksplit": 1}]
CUS = 256


def tune(sw):
    t = dict(DEFAULT, **sw)
    return [t[k] for k in ("pf32_min_t", "pf32_ks2", "pf32_paired", "pf_waves", "pf_stages", "pf_ksplit")]


def single(T, H, Hkv, d, sw={}, force=0, scale_positive=1, cus=CUS):
    return ["s", T, H, Hkv, d, force, scale_positive, cus] + tune(sw)


def packed(H, Hkv, d, counts, sw={}):
    return ["p", H, Hkv, d] + tune(sw) + [len(counts)] + list(counts)


def cases():
    out = [single(T, H, Hkv, d, sw) for H, Hkv, d in SHAPES for sw in SETS for T in LENGTHS]
    # a pinned kernel (fl_op_attention), the 32-row kernel refused for scale <= 0, another chip's snake grid, the other switches
    out += [single(T, 32, 8, 128, force=f, scale_positive=p) for T in (100, 2048) for f, p in ((2, 1), (3, 1), (3, 0))]
    out += [single(4096, 32, 8, 128, cus=304), single(512, 32, 8, 128, {"pf32_min_t": 640}), single(200, 8, 2, 128, {"pf_stages": 4})]
    counts = PACKS["64_wide_window5"][0]
    for H, Hkv, d in SHAPES + [(2, 2, 64), (2, 2, 128), (4, 2, 64), (4, 2, 128)]:
        out += [packed(H, Hkv, d, counts, sw) for sw in ({}, {"pf_waves": 8}, {"pf_ksplit": 1})] + [packed(H, Hkv, d, [c]) for c in (1, 65, 600)]
    return out


def key(c):
    return " ".join(str(v) for v in c)


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("attn_prefill_plan") / "attn_prefill_plan")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I" + CSRC, os.path.join(ROOT, "tests", "host", "attn_prefill_plan_main.cc"), "-o", exe])

    def run(cs):
        out = subprocess.run([exe] + [str(v) for c in cs for v in c], capture_output=True, text=True, check=True).stdout.splitlines()
        assert len(out) == len(cs)
        return out
    return run


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return dict(line.rstrip("\n").split(" | ") for line in f)


def test_every_case_is_the_recorded_rule(plan, golden):
    cs = cases()
    assert sorted(golden) == sorted(set(key(c) for c in cs)), "the table and the case list differ"
    bad = ["%s: recorded %s, now %s" % (key(c), golden[key(c)], got) for c, got in zip(cs, plan(cs)) if got != golden[key(c)]]
    assert not bad, "\n".join(bad[:40])


def test_anchors_derived_by_hand(plan, golden):
    """Mistral-7B and Qwen2-7B at the default switches on 256 CUs, worked out from the rule's text: fields as the program prints them"""
    want = {
        (512, 32, 8): "32 8 4 1 0 2 16 16 512 131072 32row,ks4",        # four waves per block, 2 heads per subgroup, plain grid
        (600, 32, 8): "16 1 2 2 38 8 512 65536",                        # the 577-639 gap: 16 rows, TT 1, wave pairs, two stages
        (1536, 32, 8): "32 8 2 1 1 0 24 8 512 98304 32row,ks2",         # wave pairs, paired grid
        (2048, 32, 8): "32 8 2 1 2 0 256 1 512 98304 32row,ks2",        # two rounds of items: snake
        (4096, 32, 8): "32 8 1 2 2 0 256 1 512 49152 32row",            # 8 waves, two token blocks per workgroup, snake
        (512, 28, 4): "32 8 4 1 0 2 16 16 512 131072 32row,ks4",
    }
    cs = [single(T, H, Hkv, 128) for T, H, Hkv in want]
    assert plan(cs) == list(want.values())
    assert [golden[key(c)] for c in cs] == list(want.values())


def test_packed_plan_is_the_packed_attention_tests_restatement(plan):
    """expected_tt of tests/test_gpu_packed_attention.py, on the counts of its widest pack and on every member alone"""
    counts = PACKS["64_wide_window5"][0]
    shapes = [(H, Hkv, d) for d in (64, 128) for H, Hkv in [(2, 2), (4, 2), (6, 2), (8, 1), (32, 8)]]
    want = {(2, 2): 4, (4, 2): None, (6, 2): 2, (8, 1): 1, (32, 8): None}
    got = [int(line.split()[0]) for line in plan([packed(H, Hkv, d, counts) for H, Hkv, d in shapes])]
    for (H, Hkv, d), tt in zip(shapes, got):
        w = want[(H, Hkv)] or {(4, 2): (4, 2), (32, 8): (2, 1)}[(H, Hkv)][d == 128]
        assert tt == w == expected_tt(H, Hkv, d, counts), (H, Hkv, d, tt)
    alone = plan([packed(H, Hkv, d, [c]) for H, Hkv, d in shapes for c in sorted(set(counts))])
    assert all(int(line.split()[0]) == 1 for line in alone)
