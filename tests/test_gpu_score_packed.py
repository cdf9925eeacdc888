"""fl_batch_score (Model.score_packed): several sequences scored in ONE forward.  Members of 1, 5 and 19 tokens, the third behind a
7-token cached prefix, on llama_a: every record is the score of the row the kernel read (bf16 and fp32); in fp32 every row is the
oracle's within the bound of tests/test_gpu_score.py; the caches afterwards continue like caches filled by prefill_packed; the
argument errors of fl_batch_prefill come back unchanged."""
import numpy as np
import pytest

import score_cases as sc
import synth
from test_gpu_score import check_against_oracle, check_against_rows, oracle_model, oracle_rows

pytestmark = pytest.mark.gpu
CAP = 64
NO = sc.NO_TARGET
LENS, PREFIX = [1, 5, 19], 7


@pytest.fixture(scope="module")
def fa():
    import fastllm_amd
    assert fastllm_amd.device_count() >= 1
    return fastllm_amd


@pytest.fixture(scope="module", params=["bf16", "f32"])
def env(fa, request):
    cfg = synth.CONFIGS["llama_a"]
    gm = fa.Model(cfg, synth.synth_weights(cfg), dtype=request.param)
    yield gm, cfg, request.param
    gm.close()                                   # (no stream of this module's outlives it)


def members(gm, cfg):
    """(caches, seqs, pos, prefix): the third cache already holds the prefix"""
    seqs = [synth.prompt_ids(cfg, n, seed=800 + i) for i, n in enumerate(LENS)]
    prefix = synth.prompt_ids(cfg, PREFIX, seed=899)
    caches = [gm.new_cache(CAP) for _ in LENS]
    gm.forward(caches[2], prefix, 0)
    return caches, seqs, [0, 0, PREFIX], prefix


@pytest.mark.parametrize("top_n", [0, 5])
def test_default_targets_per_member(env, top_n):
    gm, cfg, dtype = env
    caches, seqs, pos, prefix = members(gm, cfg)
    res = gm.score_packed(caches, seqs, pos=pos, top_n=top_n, want_logits=True)
    assert [len(c) for c in caches] == [1, 5, PREFIX + 19] and len(res) == 3
    for i, s in enumerate(seqs):
        assert res[i].logits.shape == (len(s), cfg["vocab_size"])
        check_against_rows(res[i], res[i].logits, sc.next_targets(s), top_n, (dtype, "member", i))
        assert np.isnan(res[i].target_logprob[-1]) and int(res[i].target_rank[-1]) == 0
    if dtype == "f32":
        om = oracle_model("llama_a")
        for i, s in enumerate(seqs):
            pre = prefix if i == 2 else prefix[:0]
            check_against_oracle(res[i], oracle_rows(om, pre, s), sc.next_targets(s), top_n, ("oracle member", i))


def test_explicit_targets_and_no_logits(env):
    gm, cfg, dtype = env
    caches, seqs, pos, _ = members(gm, cfg)
    rs = np.random.RandomState(6)
    targets = [rs.randint(0, cfg["vocab_size"], n).astype(np.uint32) for n in LENS]
    targets[1][2] = targets[2][0] = NO
    res = gm.score_packed(caches, seqs, pos=pos, top_n=3, targets=targets, want_logits=True)
    for i in range(3):
        check_against_rows(res[i], res[i].logits, targets[i], 3, (dtype, "explicit", i))
    caches2 = members(gm, cfg)[0]
    plain = gm.score_packed(caches2, seqs, pos=pos, top_n=3, targets=targets)
    for i in range(3):
        assert plain[i].logits is None
        for a, b in zip(plain[i][:4], res[i][:4]):
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_scored_caches_continue_like_prefilled_caches(env):
    gm, cfg, dtype = env
    a, seqs, pos, _ = members(gm, cfg)
    b = members(gm, cfg)[0]
    gm.score_packed(a, seqs, pos=pos, top_n=2)
    toks = gm.prefill_packed(b, seqs, pos=pos)
    assert [len(c) for c in a] == [len(c) for c in b]
    for i in range(3):
        p = len(b[i])
        assert np.array_equal(gm.decode_greedy(a[i], toks[i], p, 6), gm.decode_greedy(b[i], toks[i], p, 6)), i


def test_block_rows_switch(fa, env):
    """lm_head blocks of 8 rows over the 25 packed rows (3 full blocks + 1 row)"""
    gm, cfg, dtype = env
    caches, seqs, pos, _ = members(gm, cfg)
    try:
        fa.tune("score_rows", 8)
        got = gm.score_packed(caches, seqs, pos=pos, top_n=4, want_logits=True)
    finally:
        fa.reload_env()
    for i, s in enumerate(seqs):
        check_against_rows(got[i], got[i].logits, sc.next_targets(s), 4, (dtype, "blocks", i))
    if dtype == "f32":
        om = oracle_model("llama_a")
        check_against_oracle(got[2], oracle_rows(om, synth.prompt_ids(cfg, PREFIX, seed=899), seqs[2]), sc.next_targets(seqs[2]), 4, "blocks oracle")


def test_argument_errors_are_the_packed_prefills(fa, env):
    gm, cfg, dtype = env
    caches, seqs, pos, _ = members(gm, cfg)
    before = [len(c) for c in caches]

    def refused(code, cs, ps, pos=pos, **kw):
        with pytest.raises(fa.FastLLMError) as e:
            gm.score_packed(cs, ps, pos=pos, **kw)
        with pytest.raises(fa.FastLLMError) as e2:
            gm.prefill_packed(cs, ps, pos=pos)
        assert e.value.code == code == e2.value.code and str(e.value) == str(e2.value), (code, str(e.value), str(e2.value))
        assert [len(c) for c in caches] == before

    refused(-8, caches, [seqs[0], [], seqs[2]])                                          # an empty member
    refused(-8, [caches[0], caches[1], caches[0]], seqs)                                 # the same cache twice
    refused(-7, caches, [seqs[0], seqs[1], synth.prompt_ids(cfg, CAP - PREFIX + 1, seed=9)])   # 7 cached + 58 > 64
    try:
        fa.tune("prefill_chunk", 16)                                                     # too many tokens for one packed call
        refused(-10, caches, seqs)
    finally:
        fa.reload_env()
    with pytest.raises(fa.FastLLMError) as e:                                            # ... and the fl_score's own: the field is named
        gm.score_packed(caches, seqs, pos=pos, targets=[[0], [1, 2, 3, 4, cfg["vocab_size"]], [0] * 19])
    assert e.value.code == -8 and "targets" in str(e.value) and [len(c) for c in caches] == before
