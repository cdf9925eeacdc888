"""fl_cache_copy_prefix: a cache that took the first n positions of another behaves as that other cache truncated to n.

Equal capacities: bit for bit (same kernels, same split counts, same bytes below n; nothing reads past the length).  Different
capacities: the decode attention splits the keys differently, so the logits are held to the oracle (check_logits) and to the
equal-capacity result within 1e-2 relative L2 (the `tight` bar of test_gpu_batch.py between kernel variants); fp32 greedy ids equal."""
import numpy as np
import pytest

import synth
from oracle import oracle
from test_gpu_parity import check_logits

pytestmark = pytest.mark.gpu

MODELS = [(n, dt, 1) for n in ("llama_a", "mistral_a", "qwen2_a", "llama_mha", "llama_d100") for dt in ("bf16", "f32")] + \
         [("llama_tp4", "bf16", 2), ("llama_tp4", "f32", 2)]
P_LEN, S_LENS, CAP = 37, (1, 5, 19), 96


@pytest.fixture(scope="module")
def fa():
    import fastllm_amd
    assert fastllm_amd.device_count() >= 1, "no MI355X visible"
    return fastllm_amd


class Ctx:
    pass


@pytest.fixture(scope="module", params=MODELS, ids=["%s-%s-tp%d" % m for m in MODELS])
def ctx(request, fa):
    name, dtype, tp = request.param
    c = Ctx()
    c.name, c.dtype, c.tp, c.fa = name, dtype, tp, fa
    c.cfg = synth.CONFIGS[name]
    w = synth.synth_weights(c.cfg)
    kw = {} if tp == 1 else dict(tp_mode=fa.binding.TP_EMULATED, tp_size=tp)
    c.gm = fa.Model(c.cfg, w, dtype=dtype, **kw)
    c.om = oracle.OracleModel(c.cfg, synth.as_f32(w), round_bf16=(dtype == "bf16"))
    c.P = synth.prompt_ids(c.cfg, P_LEN, seed=11)
    c.S = synth.prompt_ids(c.cfg, max(S_LENS), seed=12)
    c.A = c.gm.new_cache(CAP)                      # the source every test copies from; never advanced
    c.gm.forward(c.A, c.P, 0)
    c.ref = {}
    return c


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def twin(c, n, s):
    """Case 1's reference, computed once per (n, suffix length) and left unchanged: a cache of the same capacity that forwarded P
    itself, truncated to n, then the suffix and eight greedy steps."""
    if (n, s) not in c.ref:
        A2 = c.gm.new_cache(CAP)
        c.gm.forward(A2, c.P, 0)
        A2.truncate(n)
        lg = c.gm.forward(A2, c.S[:s], n)
        toks = c.gm.decode_greedy(A2, oracle.argmax(lg), n + s, 8)
        c.ref[(n, s)] = (lg, toks)
    return c.ref[(n, s)]


@pytest.mark.parametrize("n", [37, 20])
def test_equal_capacities_are_bit_exact(ctx, n):
    c = ctx
    for s in S_LENS:
        lg_ref, toks_ref = twin(c, n, s)
        B = c.gm.new_cache(CAP)
        B.copy_prefix(c.A, n)
        assert len(B) == n and len(c.A) == P_LEN
        lg = c.gm.forward(B, c.S[:s], n)
        assert len(B) == n + s
        np.testing.assert_array_equal(bits(lg), bits(lg_ref), err_msg="%s n %d suffix %d" % (c.name, n, s))
        toks = c.gm.decode_greedy(B, oracle.argmax(lg), n + s, 8)         # the second step captures the graph, the rest replay it
        np.testing.assert_array_equal(toks, toks_ref)
        assert len(B) == n + s + 8


@pytest.mark.parametrize("cap", [40, 200, 3000])
def test_different_capacities_agree_with_the_oracle_and_the_equal_capacity_result(ctx, cap):
    c = ctx
    done = 0
    for n in (37, 20):
        for s in S_LENS:
            if n + s > cap:
                continue
            B = c.gm.new_cache(cap)
            B.copy_prefix(c.A, n)
            assert len(B) == n and B.capacity() == cap
            lg = c.gm.forward(B, c.S[:s], n)
            oc = c.om.new_cache(CAP)
            c.om.forward(oc, c.P[:n], 0)
            lo = c.om.forward(oc, c.S[:s], n)
            check_logits(lg, lo, c.dtype, "%s cap %d n %d suffix %d vs oracle" % (c.name, cap, n, s))
            lg_ref, toks_ref = twin(c, n, s)
            rel = np.linalg.norm(lg - lg_ref) / np.linalg.norm(lg_ref)
            assert rel <= 1e-2, "%s cap %d n %d suffix %d vs equal capacities: rel L2 %.2e" % (c.name, cap, n, s, rel)
            if c.dtype == "f32":
                assert oracle.argmax(lg) == oracle.argmax(lg_ref)
                k = min(8, cap - n - s)
                if k:
                    np.testing.assert_array_equal(c.gm.decode_greedy(B, oracle.argmax(lg), n + s, k), toks_ref[:k])
            done += 1
    assert done >= 4                                # capacity 40 still takes n = 20 with every suffix and n = 37 with one id


def test_source_is_untouched(ctx):
    c = ctx
    A = c.gm.new_cache(CAP)
    first = c.gm.forward_argmax(A, c.P, 0)
    T = c.gm.new_cache(CAP)                          # a twin that is never copied from
    assert c.gm.forward_argmax(T, c.P, 0) == first
    B = c.gm.new_cache(CAP)
    B.copy_prefix(A, 20)
    c.gm.forward(B, c.S[:5], 20)
    c.gm.decode_greedy(B, 1, 25, 8)                  # dst has advanced past what it took
    assert len(A) == P_LEN
    np.testing.assert_array_equal(c.gm.decode_greedy(A, first, P_LEN, 8), c.gm.decode_greedy(T, first, P_LEN, 8))


@pytest.mark.parametrize("n", [37, 20])
def test_reused_destination(ctx, n):
    """dst held a longer, different sequence and has its decode graph captured: after the copy it gives the fresh cache's result."""
    c = ctx
    B = c.gm.new_cache(CAP)
    other = synth.prompt_ids(c.cfg, 50, seed=13)
    c.gm.decode_greedy(B, c.gm.forward_argmax(B, other, 0), 50, 6)
    assert len(B) == 56
    for s in (5, 1):
        B.copy_prefix(c.A, n)
        assert len(B) == n
        lg_ref, toks_ref = twin(c, n, s)
        lg = c.gm.forward(B, c.S[:s], n)
        np.testing.assert_array_equal(bits(lg), bits(lg_ref))
        np.testing.assert_array_equal(c.gm.decode_greedy(B, oracle.argmax(lg), n + s, 8), toks_ref)


def test_batch_member_between_two_batch_calls(ctx):
    c = ctx
    if c.tp != 1:
        return                                       # fl_batch_* does not take an emulated tensor-parallel model
    fa, gm = c.fa, c.gm
    caches, firsts, lens = [], [], [9, 14]
    for i, n in enumerate(lens):
        k = gm.new_cache(CAP)
        firsts.append(gm.forward_argmax(k, synth.prompt_ids(c.cfg, n, seed=60 + i), 0))
        caches.append(k)
    batch = fa.Batch(gm, caches)
    out = batch.decode(firsts, lens, 5)
    firstA = oracle.argmax(gm.forward(gm.new_cache(CAP), c.P, 0))
    caches[1].copy_prefix(c.A, P_LEN)                # slot 1 starts another stream between two batch calls
    both = batch.decode([int(out[0][-1]), firstA], [lens[0] + 5, P_LEN], 6)
    single = gm.new_cache(CAP)
    single.copy_prefix(c.A, P_LEN)
    np.testing.assert_array_equal(both[1], gm.decode_greedy(single, firstA, P_LEN, 6))
    assert len(caches[1]) == P_LEN + 6


def test_errors_and_degenerate_calls(ctx):
    c = ctx
    fa, gm = c.fa, c.gm
    B = gm.new_cache(CAP)
    gm.forward(B, c.P[:9], 0)
    with pytest.raises(fa.FastLLMError) as e:
        B.copy_prefix(c.A, P_LEN + 1)                # beyond what src holds
    assert e.value.code == -8 and len(B) == 9
    small = gm.new_cache(16)
    with pytest.raises(fa.FastLLMError) as e:
        small.copy_prefix(c.A, 20)                   # beyond dst's capacity
    assert e.value.code == -7 and len(small) == 0
    other = fa.Model(c.cfg, synth.synth_weights(c.cfg), dtype=c.dtype)
    with pytest.raises(fa.FastLLMError) as e:
        other.new_cache(CAP).copy_prefix(c.A, 5)     # caches of two models
    assert e.value.code == -8 and b"different models" in fa.lib().fl_last_error()
    B.copy_prefix(c.A, 0)                            # n == 0: fl_cache_reset
    assert len(B) == 0
    gm.forward(B, c.P[:9], 0)
    B.copy_prefix(B, 4)                              # src == dst: fl_cache_truncate
    assert len(B) == 4
    with pytest.raises(fa.FastLLMError) as e:
        B.copy_prefix(B, 5)
    assert e.value.code == -8 and len(c.A) == P_LEN
