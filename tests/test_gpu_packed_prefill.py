"""fl_batch_prefill (Model.prefill_packed): several prompts in ONE forward.  Per member the call must give what a single
Model.forward of that prompt on a fresh cache gives -- logits, token, cache length and (seen through decode steps afterwards) the
K / V it wrote -- and agree with the oracle like every other path.  Bounds: test_gpu_batch.tight (1e-2 rel. L2 between two bf16
executions that sum in different orders, 2e-3 for decode steps on the same kernels) and test_gpu_parity.check_logits."""
import numpy as np
import pytest

import synth
from oracle import oracle
from test_gpu_batch import tight
from test_gpu_parity import FP32_TOL, check_logits
from test_w8_abi import dequantized_weights

pytestmark = pytest.mark.gpu

LENS = [1, 2, 15, 16, 17, 31, 33, 48, 5, 64, 7, 100]
CAP = 160
CAPS = [CAP] * len(LENS)
CAPS[3], CAPS[10] = 96, 224                                       # two caches of another capacity (another seq_alloc)


@pytest.fixture(scope="module")
def fa():
    import fastllm_amd
    assert fastllm_amd.device_count() >= 1
    return fastllm_amd


def prompts_of(cfg, lens=LENS, extra=None):
    return [synth.prompt_ids(cfg, n + (extra[i] if extra else 0), seed=700 + i) for i, n in enumerate(lens)]


def new_caches(gm, caps=CAPS):
    return [gm.new_cache(c) for c in caps]


def decode_steps_agree(gm, packed, single, tok, pos, what, lim_B=1):
    """two decode steps with the same fed token on both caches: the check of the K / V the packed launch wrote"""
    t = int(tok)
    for s in range(2):
        a, b = gm.forward(packed, [t], pos + s), gm.forward(single, [t], pos + s)
        tight(a, b, "%s decode step %d" % (what, s), B=lim_B)
        t = oracle.argmax(b)


@pytest.mark.parametrize("name", ["llama_a", "mistral_a", "mistral_win", "qwen2_a", "llama_mha", "llama_d100", "mistral_d48"])
def test_packed_bf16_matches_single_forwards_and_oracle(fa, name):
    cfg = synth.CONFIGS[name]
    w = synth.synth_weights(cfg)
    gm = fa.Model(cfg, w, dtype="bf16")
    om = oracle.OracleModel(cfg, synth.as_f32(w), round_bf16=True)
    prompts = prompts_of(cfg)
    caches = new_caches(gm)
    toks, lg = gm.prefill_packed(caches, prompts, want_logits=True)
    for i, p in enumerate(prompts):
        what = "%s member %d (%d tokens)" % (name, i, len(p))
        single = gm.new_cache(CAPS[i])
        ref = gm.forward(single, p, 0)
        tight(lg[i], ref, what + " vs single forward", B=3)
        check_logits(lg[i], om.forward(om.new_cache(CAP), p, 0), "bf16", what + " vs oracle")
        assert toks[i] == oracle.argmax(lg[i]), what
        assert len(caches[i]) == len(p), what
        decode_steps_agree(gm, caches[i], single, toks[i], len(p), what)


@pytest.mark.parametrize("name", ["llama_a", "mistral_win", "qwen2_a"])
def test_packed_fp32_matches_oracle(fa, name):
    cfg = synth.CONFIGS[name]
    w = synth.synth_weights(cfg)
    gm = fa.Model(cfg, w, dtype="f32")
    om = oracle.OracleModel(cfg, synth.as_f32(w), round_bf16=False)
    prompts = prompts_of(cfg)
    caches = new_caches(gm)
    toks, lg = gm.prefill_packed(caches, prompts, want_logits=True)
    for i, p in enumerate(prompts):
        what = "%s fp32 member %d (%d tokens)" % (name, i, len(p))
        oc = om.new_cache(CAP)
        np.testing.assert_allclose(lg[i], om.forward(oc, p, 0), atol=FP32_TOL, rtol=0, err_msg=what)
        assert toks[i] == oracle.argmax(lg[i]) and len(caches[i]) == len(p), what
        t = int(toks[i])
        for s in range(2):
            got, ref = gm.forward(caches[i], [t], len(p) + s), om.forward(oc, [t], len(p) + s)
            np.testing.assert_allclose(got, ref, atol=FP32_TOL, rtol=0, err_msg=what + " decode step %d" % s)
            t = oracle.argmax(ref)


@pytest.mark.parametrize("name", ["llama_a", "mistral_win"])
def test_packed_behind_a_cached_prefix(fa, name):
    """every member's first k tokens are forwarded alone, the rest goes through the packed call at pos = k: the cached prefix is
    unmasked, the causal / sliding-window mask runs over the call's own tokens -- as in the same two calls done singly"""
    cfg = synth.CONFIGS[name]
    w = synth.synth_weights(cfg)
    gm = fa.Model(cfg, w, dtype="bf16")
    om = oracle.OracleModel(cfg, synth.as_f32(w), round_bf16=True)
    ks = [[0, 4, 16, 33][i % 4] for i in range(len(LENS))]
    prompts = prompts_of(cfg, extra=ks)
    caps = [224] * len(LENS)
    caches, singles = new_caches(gm, caps), new_caches(gm, caps)
    for c, s, p, k in zip(caches, singles, prompts, ks):
        if k:
            gm.forward(c, p[:k], 0)
            gm.forward(s, p[:k], 0)
    toks, lg = gm.prefill_packed(caches, [p[k:] for p, k in zip(prompts, ks)], pos=ks, want_logits=True)
    for i, (p, k) in enumerate(zip(prompts, ks)):
        what = "%s member %d (%d cached + %d new)" % (name, i, k, len(p) - k)
        ref = gm.forward(singles[i], p[k:], k)
        tight(lg[i], ref, what + " vs single forwards", B=3)
        oc = om.new_cache(224)
        if k:
            om.forward(oc, p[:k], 0)
        check_logits(lg[i], om.forward(oc, p[k:], k), "bf16", what + " vs oracle")
        assert toks[i] == oracle.argmax(lg[i]) and len(caches[i]) == len(p), what
        decode_steps_agree(gm, caches[i], singles[i], toks[i], len(p), what)


def test_packed_samplers(fa):
    """every member draws with its own sampler, once: its token is op_sample of its own logits, and the stream goes on from there"""
    cfg = synth.CONFIGS["llama_a"]
    gm = fa.Model(cfg, synth.synth_weights(cfg), dtype="bf16")
    lens = [9, 17, 33, 4, 21, 40]
    prompts = prompts_of(cfg, lens)
    temps, seeds = [None, 0.8, 0.8, None, 0.8, 0.8], [0, 3, 5, 0, 3, 5]
    top_p, top_k = [None, None, 0.9, None, None, 0.9], [None, None, 40, None, None, 40]

    def draw(lg, i, draws_done):
        if temps[i] is None:
            return oracle.argmax(lg)
        return int(fa.op_sample(lg, 1, temps[i], seed=seeds[i], draws_done=draws_done, top_p=top_p[i], top_k=top_k[i])[0])

    caches, twins = new_caches(gm, [96] * len(lens)), new_caches(gm, [96] * len(lens))
    toks, lg = gm.prefill_packed(caches, prompts, temperatures=temps, seeds=seeds, top_p=top_p, top_k=top_k, want_logits=True)
    toks2 = gm.prefill_packed(twins, prompts, temperatures=temps, seeds=seeds, top_p=top_p, top_k=top_k)     # the same call again: the same caches
    np.testing.assert_array_equal(toks, toks2)
    for i, p in enumerate(prompts):
        assert toks[i] == draw(lg[i], i, 0), "member %d" % i
        got = gm.decode_sample(caches[i], int(toks[i]), len(p), 3, temps[i] if temps[i] is not None else 0.0, seed=seeds[i], draws_done=1,
                               top_p=top_p[i], top_k=top_k[i])
        t, want = int(toks[i]), []
        for s in range(3):
            t = draw(gm.forward(twins[i], [t], len(p) + s), i, 1 + s)
            want.append(t)
        np.testing.assert_array_equal(got, want, err_msg="member %d" % i)


def test_packed_refusals_modify_nothing(fa):
    from fastllm_amd import binding
    cfg = synth.CONFIGS["llama_a"]
    w = synth.synth_weights(cfg)
    gm = fa.Model(cfg, w, dtype="bf16")
    other = fa.Model(cfg, w, dtype="bf16")
    lens = [5, 17, 3]
    prompts = prompts_of(cfg, lens)
    caches = new_caches(gm, [32, 32, 32])
    gm.forward(caches[1], prompts[1][:4], 0)                     # one member already holds something
    before = [len(c) for c in caches]

    def refused(code, cs, ps, pos=None):
        with pytest.raises(fa.FastLLMError) as e:
            gm.prefill_packed(cs, ps, pos=pos)
        assert e.value.code == code and str(e.value), (code, e.value.code, str(e.value))
        assert [len(c) for c in caches] == before

    refused(-8, [caches[0], caches[1], caches[0]], prompts)                              # the same cache twice
    refused(-8, caches, [prompts[0], [], prompts[2]])                                    # an empty member
    refused(-8, caches, [prompts[0], prompts[1], [1, cfg["vocab_size"]]])                # an id outside the vocabulary
    refused(-8, [caches[0], caches[1], other.new_cache(32)], prompts)                    # a cache of another model
    refused(-7, caches, [prompts[0], synth.prompt_ids(cfg, 29, seed=9), prompts[2]], pos=[0, 4, 0])     # 4 cached + 29 > 32
    refused(-7, caches, prompts, pos=[0, cfg["max_position_embeddings"] - 3, 0])         # a position past max_position_embeddings
    g2 = fa.Model(cfg, w, dtype="bf16", tp_mode=binding.TP_EMULATED, tp_size=2)
    c2 = [g2.new_cache(32) for _ in lens]
    with pytest.raises(fa.FastLLMError) as e:
        g2.prefill_packed(c2, prompts)
    assert e.value.code == -10 and [len(c) for c in c2] == [0, 0, 0]                     # FL_ERR_UNSUPPORTED
    # nothing was half-written: the valid call gives what single forwards give
    toks, lg = gm.prefill_packed(caches, [prompts[0], prompts[1][4:], prompts[2]], pos=[0, 4, 0], want_logits=True)
    for i, p in enumerate(prompts):
        single = gm.new_cache(32)
        tight(lg[i], gm.forward(single, p, 0), "member %d after the refusals" % i, B=3)
        assert toks[i] == oracle.argmax(lg[i]) and len(caches[i]) == len(p)
        decode_steps_agree(gm, caches[i], single, toks[i], len(p), "member %d after the refusals" % i)


def test_packed_members_of_both_cache_layouts(fa):
    """caches created with the MFMA attention layout switched off sit in one call beside caches in that layout: the packed attention
    launch serves the ones, the single-sequence launches the others, on the same q / output buffers"""
    cfg = synth.CONFIGS["mistral_win"]
    gm = fa.Model(cfg, synth.synth_weights(cfg), dtype="bf16")
    prompts = prompts_of(cfg)
    caches, singles = [], []
    try:
        for i in range(len(LENS)):
            fa.tune("attn_mfma", 0 if i % 3 == 1 else 1)           # members 1, 4, 7, 10 (2, 17, 48 and 7 tokens): the plain layout
            caches.append(gm.new_cache(CAPS[i]))
            singles.append(gm.new_cache(CAPS[i]))
    finally:
        fa.tune("attn_mfma", 1)
    toks, lg = gm.prefill_packed(caches, prompts, want_logits=True)
    for i, p in enumerate(prompts):
        what = "mixed layouts, member %d (%d tokens, %s)" % (i, len(p), "plain" if i % 3 == 1 else "MFMA")
        tight(lg[i], gm.forward(singles[i], p, 0), what + " vs single forward", B=3)
        assert toks[i] == oracle.argmax(lg[i]) and len(caches[i]) == len(p), what
        decode_steps_agree(gm, caches[i], singles[i], toks[i], len(p), what)


def test_packed_on_an_e4m3_model_reads_the_bf16_image(fa):
    cfg = synth.CONFIGS["mistral_a"]
    w = synth.synth_weights(cfg)
    g8, g16 = fa.Model(cfg, w, dtype="bf16", decode_weights="e4m3"), fa.Model(cfg, dequantized_weights(w), dtype="bf16")
    prompts = prompts_of(cfg)
    caches = new_caches(g8)
    toks, lg = g8.prefill_packed(caches, prompts, want_logits=True)
    for i, p in enumerate(prompts):
        tight(lg[i], g16.forward(g16.new_cache(CAP), p, 0), "e4m3 member %d vs the bf16 model of the quantised image" % i, B=3)
        assert toks[i] == oracle.argmax(lg[i]) and len(caches[i]) == len(p)
