"""fl_batch_embed (Model.embed_packed) end to end: decoder-model embeddings -- pooled final hidden states of a packed forward,
under the causal or the full mask.

What a row is compared with.  The hidden state of a row, projected through lm_head in float64, is that row's logits; so the rows of
an FL_POOL_NONE call are checked (a) under the causal mask against the oracle's logits of the same prefixes (a row's state is that
of the prompt that ends there) and against fl_batch_prefill's logits_out on the last rows, (b) under the full mask against
tests/decoder_ref.py (anchored to the oracle on the CPU by tests/test_decoder_ref.py).
Bounds.  fp32 models: FP32_TOL (1e-3 absolute, the bar of test_gpu_parity.py).  bf16 models: the oracle-based bounds
test_gpu_parity_bf16.py applies to logits, over all rows of the pack as relative L2: the product is at least as close to fp32 as the
candle-emulated bf16 run (e_gpu <= e_cand + 1e-4) and within 1.5 times that run's own bf16 noise of it (d <= 1.5 e_cand + 1e-4); the
HF-bf16 bound of that file needs the golden HF run and exists for the golden prompt only.  No oracle runs the full mask, so a bf16
full-mask run is held to the causal pack's e_cand: the same weights, rows and roundings, only more keys per softmax.
Bit identity alone / in the pack.  The row-wise launches of a packed forward are the planner's for the call's TOTAL row count, as in
fl_batch_prefill (whose members agree with single forwards within test_gpu_batch.tight, not bit for bit, across the planner's
thresholds).  What this change adds -- the pool tail and the full-mask attention -- must not depend on the pack at all: the test
takes a member of 17 rows alone and inside a pack of 31 rows, both inside one planner regime (3 .. 32 rows), where the projections
give a row the same bits, and asks for identical bits of the embedding."""
import ctypes as C
import os

import numpy as np
import pytest

import decoder_ref
import synth
from oracle import oracle
from test_gpu_batch import tight
from test_gpu_parity import FP32_TOL

pytestmark = pytest.mark.gpu

NAMES = ["llama_a", "mistral_win", "qwen2_win", "llama_mha", "llama_d100"]
PACK = [1, 2, 17, 33, 48]
CAP = 64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def fa():
    import fastllm_amd
    assert fastllm_amd.device_count() >= 1
    return fastllm_amd


class Env:
    pass


@pytest.fixture(scope="module", params=[(n, d) for d in ("f32", "bf16") for n in NAMES], ids=lambda p: "%s-%s" % p)
def env(fa, request):
    e = Env()
    e.name, e.dtype = request.param
    e.cfg = synth.CONFIGS[e.name]
    e.w = synth.synth_weights(e.cfg)
    e.wf = synth.as_f32(e.w)
    e.gm = fa.Model(e.cfg, e.w, dtype=e.dtype)
    e.seqs = [synth.prompt_ids(e.cfg, n, seed=900 + i) for i, n in enumerate(PACK)]
    yield e
    e.gm.close()


_ORACLE = {}


def oracle_rows(e, mode):
    """[101, V]: the oracle's logits of every prefix of every member (mode 0: fp32; 2: candle-emulated bf16) -- once per model"""
    key = (e.name, mode)
    if key not in _ORACLE:
        om = oracle.OracleModel(e.cfg, e.wf, round_bf16=mode)
        _ORACLE[key] = np.stack([om.forward(om.new_cache(CAP), s[:r + 1], 0) for s in e.seqs for r in range(len(s))])
        om.close()
    return _ORACLE[key]


def fresh(e, n=len(PACK), cap=CAP):
    return [e.gm.new_cache(cap) for _ in range(n)]


def project(e, rows):
    return decoder_ref.logits(e.cfg, e.wf, rows)


def rel(a, b):
    return float(np.linalg.norm(np.asarray(a, np.float64) - b) / np.linalg.norm(b))


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def check_rows(e, got, ref, what):
    """got / ref [rows, V]: logits from the device's hidden states against the reference's, under the dtype's bound"""
    if e.dtype == "f32":
        err = np.abs(got - ref).max()
        print("%s %s f32: max |err| %.3g (bound %.3g)" % (e.name, what, err, FP32_TOL))
        assert err <= FP32_TOL, (what, err)
        return
    ref32, cand = oracle_rows(e, 0), oracle_rows(e, 2)
    e_cand = rel(cand, ref32)
    e_gpu = rel(got, ref)
    print("%s %s bf16: rel L2 to the reference %.3g, candle-emulated bf16 %.3g" % (e.name, what, e_gpu, e_cand))
    assert e_gpu <= e_cand + 1e-4, (what, e_gpu, e_cand)
    if ref is ref32:
        d = rel(got, cand)
        print("%s %s bf16: rel L2 to the candle-emulated run %.3g (bound %.3g)" % (e.name, what, d, 1.5 * e_cand + 1e-4))
        assert d <= 1.5 * e_cand + 1e-4, (what, d, e_cand)


def test_causal_rows_are_the_oracles(env):
    e = env
    caches = fresh(e)
    rows = e.gm.embed_packed(caches, e.seqs, pooling="none", normalize=False)
    assert rows.shape == (sum(PACK), e.cfg["hidden_size"]) and np.isfinite(rows).all()
    assert [len(c) for c in caches] == PACK
    ref = oracle_rows(e, 0)
    check_rows(e, project(e, rows), ref, "causal rows vs oracle")
    # ... and the last rows against fl_batch_prefill's own logits of the same pack
    _, lg = e.gm.prefill_packed(fresh(e), e.seqs, want_logits=True)
    last = np.cumsum(PACK) - 1
    mine = project(e, rows[last])
    if e.dtype == "f32":
        assert np.abs(mine - lg).max() <= FP32_TOL
    else:
        e_cand = rel(oracle_rows(e, 2), ref)
        assert rel(mine, lg.astype(np.float64)) <= 1.5 * e_cand + 1e-4       # two bf16 runs of one forward; only lm_head differs


def test_full_mask_rows_are_the_references(env):
    e = env
    rows = e.gm.embed_packed(fresh(e), e.seqs, pooling="none", mask="full", normalize=False)
    ref_h = np.concatenate([decoder_ref.hidden_states(e.cfg, e.wf, s, mask="full") for s in e.seqs])
    ref = project(e, ref_h)
    check_rows(e, project(e, rows), ref, "full-mask rows vs decoder_ref")
    if "sliding_window" in e.cfg:
        nowin = dict(e.cfg, sliding_window=None)                  # the window is not applied
        assert np.array_equal(ref_h, np.concatenate([decoder_ref.hidden_states(nowin, e.wf, s, mask="full") for s in e.seqs]))
    # the mask is really off: row 0 of the 17-token member is not its causal value
    causal = e.gm.embed_packed(fresh(e), e.seqs, pooling="none", normalize=False)
    r0 = PACK[0] + PACK[1]
    a, b = project(e, rows[r0:r0 + 1]), project(e, causal[r0:r0 + 1])
    if e.dtype == "f32":
        assert np.abs(a - b).max() > 10 * FP32_TOL
    else:
        assert rel(a, b) > 10 * (rel(oracle_rows(e, 2), oracle_rows(e, 0)) + 1e-4)
    # one-token members see their one key under both masks
    assert np.array_equal(bits(rows[0]), bits(causal[0]))


@pytest.mark.parametrize("mask", ["causal", "full"])
def test_pooling_is_the_restatement_on_the_calls_own_rows(env, mask):
    e = env
    rows = e.gm.embed_packed(fresh(e), e.seqs, pooling="none", mask=mask, normalize=False)
    for pooling in ("last", "first", "mean"):
        want = decoder_ref.pool_f32(rows, PACK, pooling, 40)
        got = e.gm.embed_packed(fresh(e), e.seqs, pooling=pooling, mask=mask, normalize=False, dimensions=40)
        assert got.shape == (len(PACK), 40)
        assert np.array_equal(bits(got), bits(want)), (pooling, np.abs(got - want).max())
        norm = e.gm.embed_packed(fresh(e), e.seqs, pooling=pooling, mask=mask, normalize=True, dimensions=40)
        decoder_ref.check_normalized(norm, want, "%s %s %s" % (e.name, mask, pooling))
        full = e.gm.embed_packed(fresh(e), e.seqs, pooling=pooling, mask=mask, normalize=True)
        decoder_ref.check_normalized(full, decoder_ref.pool_f32(rows, PACK, pooling), "%s %s %s all columns" % (e.name, mask, pooling))
    none_norm = e.gm.embed_packed(fresh(e), e.seqs, pooling="none", mask=mask, normalize=True, dimensions=40)
    decoder_ref.check_normalized(none_norm, rows[:, :40], "%s %s none" % (e.name, mask))


@pytest.mark.parametrize("mask", ["causal", "full"])
def test_a_members_embedding_has_the_same_bits_alone_and_in_the_pack(env, mask):
    e = env
    seqs = [synth.prompt_ids(e.cfg, n, seed=950 + i) for i, n in enumerate([5, 17, 9])]        # 31 rows; the member alone: 17
    for pooling in ("last", "mean"):
        pack = e.gm.embed_packed(fresh(e, 3), seqs, pooling=pooling, mask=mask)
        alone = e.gm.embed_packed(fresh(e, 1), seqs[1:2], pooling=pooling, mask=mask)
        moved = e.gm.embed_packed(fresh(e, 3), seqs[::-1], pooling=pooling, mask=mask)
        n_diff = int((bits(pack[1]) != bits(alone[0])).sum())
        print("%s %s %s %s: %d of %d elements differ alone / in the pack, max |diff| %.3g" % (
            e.name, e.dtype, mask, pooling, n_diff, pack.shape[1], np.abs(pack[1] - alone[0]).max()))
        assert np.array_equal(bits(pack[1]), bits(moved[1])), "the member changes with its place in the pack"
        assert n_diff == 0


def test_after_a_causal_call_the_caches_are_a_prefills(env):
    e = env
    a, b = fresh(e), fresh(e)
    e.gm.embed_packed(a, e.seqs, pooling="mean")
    toks = e.gm.prefill_packed(b, e.seqs)
    assert [len(c) for c in a] == [len(c) for c in b] == PACK
    for i, n in enumerate(PACK):
        k = min(8, CAP - n)
        assert np.array_equal(e.gm.decode_greedy(a[i], int(toks[i]), n, k), e.gm.decode_greedy(b[i], int(toks[i]), n, k)), i


def test_a_cached_prefix_is_attended_to_but_not_pooled(env):
    """fl_cache_copy_prefix of a 16-token instruction, then the 9-token continuation: the last 9 rows of embedding all 25 tokens,
    within the agreement of the prefix tests (rel. L2 1e-2)"""
    e = env
    both = synth.prompt_ids(e.cfg, 25, seed=77)
    src = e.gm.new_cache(CAP)
    e.gm.forward(src, both[:16], 0)                               # the shared instruction
    c = e.gm.new_cache(CAP)
    c.copy_prefix(src, 16)
    for pooling in ("last", "mean", "none"):
        c.copy_prefix(src, 16)
        got = e.gm.embed_packed([c], [both[16:]], pos=[16], pooling=pooling, normalize=False)
        assert len(c) == 25
        if (e.cfg.get("sliding_window") or 10 ** 9) >= 25:
            whole = e.gm.embed_packed(fresh(e, 1), [both], pooling="none", normalize=False)[16:]
        else:
            # a window that bites runs over a call's own tokens, the cached prefix is unmasked (App. A.5, as in fl_forward): one call
            # over all 25 tokens is another computation.  The comparison is with those two calls made on one cache, and (fp32) with
            # their restatement in decoder_ref.
            two = e.gm.new_cache(CAP)
            e.gm.forward(two, both[:16], 0)
            whole = e.gm.embed_packed([two], [both[16:]], pos=[16], pooling="none", normalize=False)
            if e.dtype == "f32":
                ref = decoder_ref.hidden_states(e.cfg, e.wf, both, call0=16)[16:]
                assert np.abs(project(e, whole) - project(e, ref)).max() <= FP32_TOL
        want = whole if pooling == "none" else decoder_ref.pool_f32(whole, [9], pooling)
        assert got.shape == want.shape
        r = rel(got, want.astype(np.float64))
        print("%s %s prefix, %s: rel L2 %.3g" % (e.name, e.dtype, pooling, r))
        assert r <= 1e-2                                          # the kernel variants' agreement of the prefix tests


@pytest.fixture(scope="module", params=["f32", "bf16"])
def env_a(fa, request):
    """llama_a in both dtypes: the tests of argument handling need one model per dtype, not every architecture"""
    e = Env()
    e.name, e.dtype = "llama_a", request.param
    e.cfg = synth.CONFIGS[e.name]
    e.w = synth.synth_weights(e.cfg)
    e.gm = fa.Model(e.cfg, e.w, dtype=e.dtype)
    e.seqs = [synth.prompt_ids(e.cfg, n, seed=900 + i) for i, n in enumerate(PACK)]
    yield e
    e.gm.close()


def test_refusals_leave_the_caches_alone(fa, env_a):
    e = env_a
    caches = fresh(e)
    e.gm.forward(caches[1], e.seqs[1][:1], 0)                     # one member already holds a token
    before = [len(c) for c in caches]

    def refused(code, cs, ps, word=None, **kw):
        with pytest.raises(fa.FastLLMError) as ex:
            e.gm.embed_packed(cs, ps, **kw)
        assert ex.value.code == code and (word is None or word in str(ex.value)), (code, ex.value.code, str(ex.value))
        assert [len(c) for c in caches] == before

    refused(-10, caches, e.seqs, "FL_MASK_FULL", mask="full")                             # FULL on a cache that is not empty
    refused(-8, caches, e.seqs, "dimensions", dimensions=e.cfg["hidden_size"] + 1)
    refused(-8, caches, e.seqs, "pooling", pooling=4)
    refused(-8, caches, e.seqs, "mask", mask=2)
    refused(-8, [caches[0], caches[1], caches[0], caches[3], caches[4]], e.seqs)          # the same cache twice
    refused(-8, caches, [e.seqs[0], [], e.seqs[2], e.seqs[3], e.seqs[4]])                 # an empty member
    many = [e.gm.new_cache(8) for _ in range(65)]
    for call in (e.gm.embed_packed, e.gm.prefill_packed):                                # 65 members: as fl_batch_prefill
        with pytest.raises(fa.FastLLMError) as ex:
            call(many, [[1]] * 65)
        assert ex.value.code == -8 and [len(c) for c in many] == [0] * 65
    big = [e.gm.new_cache(256) for _ in range(64)]
    toks = [synth.prompt_ids(e.cfg, 128 + (i == 0), seed=i) for i in range(64)]           # 8193 tokens
    msgs = []
    for call in (e.gm.embed_packed, e.gm.prefill_packed):
        with pytest.raises(fa.FastLLMError) as ex:
            call(big, toks)
        msgs.append((ex.value.code, str(ex.value)))
        assert [len(c) for c in big] == [0] * 64
    assert msgs[0][0] == msgs[1][0] == -10 and all("8193 tokens" in m and "at most 8192" in m for _, m in msgs)
    assert "fl_batch_embed" in msgs[0][1] and "fl_batch_embed" not in msgs[1][1]     # the same limit, each call under its own name
    g2 = fa.Model(e.cfg, e.w, dtype=e.dtype, tp_mode=fa.binding.TP_EMULATED, tp_size=2)   # an emulated-TP model
    c2 = [g2.new_cache(CAP) for _ in PACK]
    with pytest.raises(fa.FastLLMError) as ex:
        g2.embed_packed(c2, e.seqs)
    assert ex.value.code == -10 and [len(c) for c in c2] == [0] * len(PACK)
    g2.close()
    # nothing was half-done: the valid call still gives what a fresh pack gives
    got = e.gm.embed_packed(caches, [e.seqs[0], e.seqs[1][1:]] + e.seqs[2:], pos=[0, 1, 0, 0, 0], pooling="none", normalize=False)
    assert [len(c) for c in caches] == PACK and np.isfinite(got).all()


def test_logit_rules_are_ignored_and_left_alone(env_a):
    e = env_a
    a, b = fresh(e), fresh(e)
    a[2].set_logit_rules(prompt_ids=e.seqs[2], logit_bias={3: -5.0}, repetition_penalty=1.3)
    words = a[2].logit_counts().copy()
    assert np.array_equal(bits(e.gm.embed_packed(a, e.seqs)), bits(e.gm.embed_packed(b, e.seqs)))
    assert np.array_equal(a[2].logit_counts(), words)


def test_an_e4m3_model_embeds_through_the_bf16_image(fa):
    from test_w8_abi import dequantized_weights
    cfg = synth.CONFIGS["mistral_a"]
    w = synth.synth_weights(cfg)
    g8, g16 = fa.Model(cfg, w, dtype="bf16", decode_weights="e4m3"), fa.Model(cfg, dequantized_weights(w), dtype="bf16")
    seqs = [synth.prompt_ids(cfg, n, seed=900 + i) for i, n in enumerate(PACK)]
    for mask in ("causal", "full"):
        a = g8.embed_packed([g8.new_cache(CAP) for _ in PACK], seqs, mask=mask, pooling="mean")
        b = g16.embed_packed([g16.new_cache(CAP) for _ in PACK], seqs, mask=mask, pooling="mean")
        for i in range(len(PACK)):
            tight(a[i], b[i], "e4m3 member %d (%s) vs the bf16 model of the quantised image" % (i, mask), B=3)
    g8.close()
    g16.close()


# ---- the C++ mirror (DecoderEmbeddingModel) through host_capi --------------------------------------------------------------------
@pytest.fixture(scope="module")
def host():
    L = C.CDLL(os.path.join(ROOT, "fastllm_amd", "lib", "libfastllm_host.so"))
    vp, sz = C.c_void_p, C.c_size_t
    L.flh_last_error.restype = C.c_char_p
    L.flh_decoder_embedding_create_on.argtypes = [vp, C.c_int, C.c_int, C.c_int, sz, sz, sz, C.POINTER(vp)]
    L.flh_decoder_embedding_destroy.argtypes = [vp]
    L.flh_decoder_embedding_destroy.restype = None
    L.flh_decoder_embedding_size.argtypes = [vp]
    L.flh_decoder_embedding_size.restype = sz
    L.flh_decoder_embedding_calls.argtypes = [vp]
    L.flh_decoder_embedding_calls.restype = sz
    L.flh_decoder_embed_batch_ids.argtypes = [vp, vp, vp, sz, vp]
    L.flh_decoder_embed_ids.argtypes = [vp, vp, sz, vp, C.POINTER(sz)]
    L.flh_decoder_compute_similarity_ids.argtypes = [vp, vp, sz, vp, sz, C.POINTER(C.c_float)]
    return L


@pytest.mark.parametrize("pooling,mask", [("last", "causal"), ("mean", "full")])
def test_the_cpp_mirror_splits_70_sequences_over_a_64_slot_pool(fa, host, pooling, mask):
    cfg = synth.CONFIGS["llama_a"]
    gm = fa.Model(cfg, synth.synth_weights(cfg), dtype="bf16")
    seqs = [synth.prompt_ids(cfg, 3 + (i * 5) % 14, seed=300 + i) for i in range(70)]
    h = C.c_void_p()
    assert host.flh_decoder_embedding_create_on(gm._h, fa.POOLING[pooling], fa.ATTN_MASK[mask], 1, 0, 64, 32, C.byref(h)) == 0, host.flh_last_error()
    dims = host.flh_decoder_embedding_size(h)
    assert dims == cfg["hidden_size"]
    ids = np.concatenate(seqs).astype(np.uint32)
    offs = np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.uint64)
    out = np.full((70, dims), np.nan, np.float32)
    assert host.flh_decoder_embed_batch_ids(h, ids.ctypes.data, offs.ctypes.data, 70, out.ctypes.data) == 0, host.flh_last_error()
    assert host.flh_decoder_embedding_calls(h) == 2 and np.isfinite(out).all()
    # the same two calls made by hand: the same bits
    pool = [gm.new_cache(32) for _ in range(64)]
    first = gm.embed_packed(pool, seqs[:64], pooling=pooling, mask=mask)
    for c in pool:
        c.reset()
    second = gm.embed_packed(pool[:6], seqs[64:], pooling=pooling, mask=mask)
    assert np.array_equal(bits(out), bits(np.concatenate([first, second])))
    # ... and 70 single calls: the planner's kernels for one short prompt, within the agreement of two bf16 runs that sum in other orders
    one = np.zeros(dims, np.float32)
    n_tok = C.c_size_t(0)
    for i, s in enumerate(seqs):
        a = np.ascontiguousarray(s, np.uint32)
        assert host.flh_decoder_embed_ids(h, a.ctypes.data, a.size, one.ctypes.data, C.byref(n_tok)) == 0, host.flh_last_error()
        assert n_tok.value == len(s)
        tight(out[i], one, "sequence %d in the pool vs alone" % i, B=3)
    sim = C.c_float(0)
    a = np.ascontiguousarray(seqs[5], np.uint32)
    assert host.flh_decoder_compute_similarity_ids(h, a.ctypes.data, a.size, a.ctypes.data, a.size, C.byref(sim)) == 0
    assert abs(sim.value - 1.0) <= 1e-6
    host.flh_decoder_embedding_destroy(h)
    gm.close()
