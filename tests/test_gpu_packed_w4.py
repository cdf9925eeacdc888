"""Packed forwards of 2-128 rows of an MXFP4 model (decode_weights="mxfp4") under fl_tune "rows_w4" read the e2m1 nibbles
(k_gemm_rows_w4.hip, k_gemm_rows64_w4.hip and, from 65 rows, k_gemm_rows128_w4.hip).  As in tests/test_gpu_rows_w4_model.py: with the
switch off (the default) the rows are the bf16 model's of W' = 2^e * q bit for bit; with it on they differ in fp32 summation order
only, and are held to the rule the project has for two such executions."""
import numpy as np
import pytest

import synth
from test_gpu_batch_w8 import rel
from test_gpu_rows_w4_model import models
from test_gpu_verify import expected

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fa():
    import fastllm_amd
    assert fastllm_amd.device_count() >= 1
    return fastllm_amd


def w4_launches(m, run, rows):
    """run(), the launches of the w4 row kernels in it, and those among them that ran the whole pack of `rows` rows (the layers'
    projections: the profile name carries the row count, the lm_head of a prefill's n last rows has another)"""
    m.profile_begin()
    out = run()
    w4 = [s for s in m.profile_end() if "[rows" in s["name"] and ",w4]" in s["name"]]
    return out, sum(s["launches"] for s in w4), sum(s["launches"] for s in w4 if "[rows%d," % rows in s["name"])


# members x tokens: 12, 40, 72 and 128 rows -- one pack per row kernel and the full height; Qwen2 for the q/k/v bias in the RoPE launch
@pytest.mark.parametrize("name,n,t", [("mistral_a", 3, 4), ("mistral_a", 5, 8), ("mistral_a", 9, 8), ("mistral_a", 8, 16), ("qwen2_a", 9, 8)])
def test_packed_prefill_streams_the_nibbles(fa, name, n, t):
    cfg, g4, g16, om = models(fa, name)
    prompts = [synth.prompt_ids(cfg, t, seed=500 + i) for i in range(n)]

    def run(m, switch):
        fa.tune("rows_w4", switch)
        caches = [m.new_cache(64) for _ in range(n)]
        (_, lg), n_w4, n_pack = w4_launches(m, lambda: m.prefill_packed(caches, prompts, want_logits=True), n * t)
        assert [len(c) for c in caches] == [t] * n
        # the layers' projections themselves: on the nibbles up to 80 rows (from 65: k_gemm_rows128_w4.hip), on the image beyond
        assert n_pack == (0 if switch == 0 or m is g16 or n * t > 80 else 4 * cfg["num_hidden_layers"])
        return lg, n_w4

    try:
        (on, n_on), (off, n_off), (ref16, _) = run(g4, 1), run(g4, 0), run(g16, 1)
    finally:
        fa.tune("rows_w4", 0)
    ref = np.stack([om.forward(om.new_cache(64), p, 0) for p in prompts])
    assert np.array_equal(off, ref16) and n_off == 0                         # switch 0: the launches of the bf16 image
    assert not np.array_equal(on, off) and n_on > 0                          # switch 1: other kernels, another summation order
    e4, e16 = rel(on, ref), rel(ref16, ref)
    print("\n%s %d x %d rows: rel L2 to fp32 on W' -- mxfp4 pack %.3e, bf16 %.3e, %d w4 launches" % (name, n, t, e4, e16, n_on))
    assert e4 <= 1.5 * e16 + 1e-4, (e4, e16)
    g4.close(); g16.close()


def test_packed_verify_streams_the_nibbles(fa):
    """9 members x (1 + 7) rows = 72.  fl_batch_verify hands the raw rows back, so the ids and accepted counts under the switch are
    held to what expected() derives from THAT run's own logits (not to the switch-0 run's)."""
    cfg, g4, g16, _ = models(fa, "mistral_a")
    n, L, nd = 9, 9, 7
    prompts = [synth.prompt_ids(cfg, L, seed=600 + i) for i in range(n)]
    firsts, drafts = [], []
    for p in prompts:                                                        # the bf16 model's own continuation with one wrong id
        c = g16.new_cache(64)
        firsts.append(g16.forward_argmax(c, p, 0))
        d = np.array(g16.decode_greedy(c, firsts[-1], L, nd), np.uint32)
        d[nd // 2] = (d[nd // 2] + 1) % cfg["vocab_size"]
        drafts.append(d)

    def step(m, switch):
        fa.tune("rows_w4", switch)
        caches = [m.new_cache(64) for _ in range(n)]
        assert [m.forward_argmax(c, p, 0) for c, p in zip(caches, prompts)] == firsts       # (prompts run on the image in both models)
        (got, lg), n_w4, n_pack = w4_launches(m, lambda: m.verify_packed(caches, firsts, drafts, [L] * n, want_logits=True), n * (nd + 1))
        assert n_pack == (4 * cfg["num_hidden_layers"] + 1 if switch == 1 and m is g4 else 0)     # every projection and the lm_head block
        for i in range(n):
            rows = lg[i * (nd + 1): (i + 1) * (nd + 1)]
            assert got[i].tolist() == expected(rows, drafts[i]) and len(caches[i]) == L + len(got[i])
        return lg, n_w4

    try:
        (on, n_on), (off, n_off), (ref16, _) = step(g4, 1), step(g4, 0), step(g16, 1)
    finally:
        fa.tune("rows_w4", 0)
    assert np.array_equal(off, ref16) and n_off == 0
    assert not np.array_equal(on, off) and n_on > 0
    g4.close(); g16.close()
