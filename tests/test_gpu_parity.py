"""GPU parity tests: the HIP path, called through the C ABI, against the CPU oracle.

Bar (BASELINE.json north_star): logits within 1e-3 of the reference CPU provider in fp32;
greedy token ids identical.  The bf16 production path is compared with the oracle run in
bf16-emulation mode (same rounding points) and, margin-aware, with the fp32 oracle.
"""
import json
import os

import numpy as np
import pytest

import synth
from conftest import needs_experimental
from oracle import oracle

pytestmark = pytest.mark.gpu

FP32_TOL = 1e-3          # north_star: "within 1e-3 fp32" (absolute, logits of magnitude O(1-10))
# bf16 path vs the oracle with the same bf16 rounding points: what is left is summation order and
# 1-ulp bf16 flips (2^-9 relative each) that propagate; bounded relative to the logit scale.
BF16_REL_MAX = 2e-2      # max |diff| <= 2e-2 * max |ref|
BF16_REL_L2 = 1e-2       # ||diff||_2 <= 1e-2 * ||ref||_2


def check_logits(got, ref, dtype, msg=""):
    if dtype == "f32":
        np.testing.assert_allclose(got, ref, atol=FP32_TOL, rtol=0, err_msg=msg)
    else:
        d = np.abs(got - ref)
        assert d.max() <= BF16_REL_MAX * max(1.0, np.abs(ref).max()), "%s max diff %g" % (msg, d.max())
        assert np.linalg.norm(got - ref) <= BF16_REL_L2 * np.linalg.norm(ref), "%s rel L2 %g" % (
            msg, np.linalg.norm(got - ref) / np.linalg.norm(ref))

CASES = ["llama_a", "llama_mha", "mistral_a", "mistral_win", "qwen2_a", "qwen2_win", "llama_d100", "qwen2_d96", "mistral_d48"]


@pytest.fixture(scope="module")
def fa():
    import fastllm_amd
    assert fastllm_amd.device_count() >= 1, "no MI355X visible"
    return fastllm_amd


@pytest.fixture(scope="module", params=CASES)
def case(request, fa):
    cfg = synth.CONFIGS[request.param]
    w = synth.synth_weights(cfg)
    return request.param, cfg, w


def _models(fa, cfg, w, dtype):
    gm = fa.Model(cfg, w, dtype=dtype)
    om = oracle.OracleModel(cfg, synth.as_f32(w), round_bf16=(dtype == "bf16"))
    return gm, om


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_prefill_then_decode_logits(fa, case, dtype):
    name, cfg, w = case
    gm, om = _models(fa, cfg, w, dtype)
    T = 24
    ids = synth.prompt_ids(cfg, T + 12, seed=7)
    gc, oc = gm.new_cache(64), om.new_cache(64)
    lg, lo = gm.forward(gc, ids[:T], 0), om.forward(oc, ids[:T], 0)
    assert len(gc) == len(oc) == T
    check_logits(lg, lo, dtype, "prefill")
    for i in range(12):                      # teacher-forced decode: same inputs on both sides
        lg, lo = gm.forward(gc, ids[T + i:T + i + 1], T + i), om.forward(oc, ids[T + i:T + i + 1], T + i)
        check_logits(lg, lo, dtype, "decode step %d" % i)
    assert len(gc) == T + 12


def test_golden_vectors_fp32(fa, case, golden_dir):
    """fp32 HIP path against the HF-generated fixtures directly."""
    name, cfg, w = case
    z = np.load(os.path.join(golden_dir, name + ".npz"))
    meta = json.loads(bytes(z["meta"]).decode())
    gm = fa.Model(cfg, w, dtype="f32")
    c = gm.new_cache(64)
    np.testing.assert_allclose(gm.forward(c, z["prompt"], 0), z["prefill_logits"], atol=FP32_TOL, rtol=0)
    if meta["n_gen"]:
        toks = []
        pos = meta["T"]
        tok = int(np.argmax(z["prefill_logits"]))
        for i in range(meta["n_gen"]):
            toks.append(tok)
            if i + 1 == meta["n_gen"]:
                break
            lg = gm.forward(c, [tok], pos)
            np.testing.assert_allclose(lg, z["gen_logits"][i + 1], atol=FP32_TOL, rtol=0)
            pos += 1
            tok = oracle.argmax(lg)
        np.testing.assert_array_equal(np.array(toks, dtype=np.uint32), z["gen_tokens"])


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_kv_cache_equivalence(fa, case, dtype):
    """prefill(T) == prefill(T-k) + k decode steps (same rounding points in both paths)."""
    name, cfg, w = case
    if name in ("mistral_win", "qwen2_win"):
        pytest.skip("decode has no window (App. A.5): the two differ by construction")
    gm = fa.Model(cfg, w, dtype=dtype)
    ids = synth.prompt_ids(cfg, 20, seed=3)
    c1, c2 = gm.new_cache(32), gm.new_cache(32)
    full = gm.forward(c1, ids, 0)
    gm.forward(c2, ids[:15], 0)
    for i in range(15, 20):
        part = gm.forward(c2, ids[i:i + 1], i)
    if dtype == "f32":
        np.testing.assert_allclose(part, full, atol=2e-4, rtol=0)
    else:
        check_logits(part, full, dtype, "prefill vs prefill+decode")


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_greedy_decode_tokens(fa, case, dtype):
    """Device-side greedy loop vs the oracle's generate(): identical ids (margin-aware for bf16)."""
    name, cfg, w = case
    if name == "mistral_win":
        pytest.skip("prefill-only config")
    gm, om = _models(fa, cfg, w, dtype)
    T, n = 8, 24
    ids = synth.prompt_ids(cfg, T)
    oc = om.new_cache(64)
    otoks, ologits = om.generate(oc, ids, n, want_logits=True)
    gc = gm.new_cache(64)
    first = gm.forward_argmax(gc, ids, 0)
    rest = gm.decode_greedy(gc, first, T, n - 1)
    gtoks = np.concatenate([[first], rest]).astype(np.uint32)
    if dtype == "f32":
        np.testing.assert_array_equal(gtoks, otoks)
    else:
        # same token wherever the oracle's top-2 margin exceeds the bf16 tolerance; stop at the
        # first legitimate divergence (after it the two sequences are different problems)
        for i in range(n):
            if gtoks[i] != otoks[i]:
                top2 = np.sort(ologits[i])[-2:]
                lim = 2 * BF16_REL_MAX * max(1.0, np.abs(ologits[i]).max())
                assert top2[1] - top2[0] < lim, "token %d differs with margin %g" % (i, top2[1] - top2[0])
                break
    assert len(gc) == T + n - 1


def test_argmax_tie_break_last_index(fa):
    """LogitsProcessor ArgMax = max_by(total_cmp): the LAST maximal index wins (App. A.7)."""
    cfg = dict(synth.CONFIGS["llama_mha"])
    w = synth.synth_weights(cfg)
    # duplicate lm_head rows -> exactly tied logits
    lm = w["lm_head.weight"].copy()
    lm[150] = lm[17]
    lm[199] = lm[17]
    w["lm_head.weight"] = lm
    gm = fa.Model(cfg, w, dtype="f32")
    om = oracle.OracleModel(cfg, synth.as_f32(w))
    ids = synth.prompt_ids(cfg, 6)
    lo = om.forward(om.new_cache(16), ids, 0)
    assert lo[17] == lo[150] == lo[199]
    # make the tied value the maximum by checking both sides agree whatever it is
    tok = gm.forward_argmax(gm.new_cache(16), ids, 0)
    assert tok == oracle.argmax(lo)
    # forced tie at the top: identical rows everywhere
    lm[:] = lm[17]
    w["lm_head.weight"] = lm
    gm2 = fa.Model(cfg, w, dtype="f32")
    assert gm2.forward_argmax(gm2.new_cache(16), ids, 0) == cfg["vocab_size"] - 1


def test_errors(fa):
    cfg = dict(synth.CONFIGS["llama_a"])
    w = synth.synth_weights(cfg)
    gm = fa.Model(cfg, w, dtype="bf16")
    c = gm.new_cache(8)
    with pytest.raises(fa.FastLLMError) as e:
        gm.forward(c, np.arange(9) % 7, 0)
    assert e.value.code == -7                                  # FL_ERR_SEQ_OVERFLOW
    with pytest.raises(fa.FastLLMError) as e:
        gm.forward(c, [cfg["vocab_size"]], 0)
    assert e.value.code == -8                                  # FL_ERR_BAD_ARGUMENT
    w2 = dict(w)
    del w2["model.layers.1.mlp.up_proj.weight"]
    with pytest.raises(fa.FastLLMError) as e:
        fa.Model(cfg, w2)
    assert e.value.code == -2 and "up_proj" in str(e.value)    # FL_ERR_MISSING_TENSOR
    bad = dict(cfg, num_attention_heads=3)
    with pytest.raises(fa.FastLLMError) as e:
        fa.Model(bad, w)
    assert e.value.code == -1                                  # FL_ERR_BAD_CONFIG
    # cache reuse after reset gives the same answer
    c.reset()
    a = gm.forward(c, [1, 2, 3], 0)
    c.reset()
    b = gm.forward(c, [1, 2, 3], 0)
    np.testing.assert_array_equal(a, b)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("name,tp", [("llama_a", 2), ("mistral_a", 2), ("qwen2_a", 2), ("llama_mha", 2), ("llama_d100", 2), ("qwen2_d96", 2)])
def test_tensor_parallel_emulated(fa, name, tp, dtype):
    """TP=N shards (row/column split + all-reduce after o_proj / down_proj + vocab all-gather) run on
    one GPU with local collectives must reproduce TP=1 (to summation-order tolerance)."""
    from fastllm_amd import binding
    cfg = synth.CONFIGS[name]
    w = synth.synth_weights(cfg)
    g1 = fa.Model(cfg, w, dtype=dtype)
    gN = fa.Model(cfg, w, dtype=dtype, tp_mode=binding.TP_EMULATED, tp_size=tp)
    om = oracle.OracleModel(cfg, synth.as_f32(w), round_bf16=(dtype == "bf16"))
    ids = synth.prompt_ids(cfg, 14, seed=11)
    c1, cN, oc = g1.new_cache(32), gN.new_cache(32), om.new_cache(32)
    a, b, o = g1.forward(c1, ids[:10], 0), gN.forward(cN, ids[:10], 0), om.forward(oc, ids[:10], 0)
    check_logits(b, o, dtype, "tp prefill vs oracle")
    if dtype == "f32":
        np.testing.assert_allclose(b, a, atol=2e-4, rtol=0)
    for i in range(10, 14):
        a, b, o = g1.forward(c1, ids[i:i + 1], i), gN.forward(cN, ids[i:i + 1], i), om.forward(oc, ids[i:i + 1], i)
        check_logits(b, o, dtype, "tp decode vs oracle")
        if dtype == "f32":
            np.testing.assert_allclose(b, a, atol=2e-4, rtol=0)
    # device-side greedy loop under TP
    f = gN.forward_argmax(cN, ids[:1], 14)
    rest = gN.decode_greedy(cN, f, 15, 4)
    assert len(rest) == 4 and len(cN) == 19


def test_unfused_decode_path_matches_fused(fa, monkeypatch):
    cfg = synth.CONFIGS["mistral_a"]
    w = synth.synth_weights(cfg)
    ids = synth.prompt_ids(cfg, 9)
    outs = []
    for fused in ("1", "0"):
        monkeypatch.setenv("FL_FUSED", fused)
        gm = fa.Model(cfg, w, dtype="f32")
        c = gm.new_cache(32)
        gm.forward(c, ids[:8], 0)
        outs.append(gm.forward(c, ids[8:9], 8))
    np.testing.assert_allclose(outs[0], outs[1], atol=1e-5, rtol=0)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("name", ["llama_a", "mistral_a", "qwen2_a"])
def test_decode_split_s_path(fa, name, dtype):
    """Cache capacity > 2048 positions makes the decode attention split S across workgroups and
    combine in-launch (ticket + release/acquire); results must not depend on the split."""
    cfg = synth.CONFIGS[name]
    w = synth.synth_weights(cfg)
    gm, om = _models(fa, cfg, w, dtype)
    ids = synth.prompt_ids(cfg, 40, seed=5)
    big, small, oc = gm.new_cache(7000), gm.new_cache(64), om.new_cache(64)
    gm.forward(big, ids[:30], 0); gm.forward(small, ids[:30], 0); om.forward(oc, ids[:30], 0)
    for i in range(30, 40):
        a = gm.forward(big, ids[i:i + 1], i)
        b = gm.forward(small, ids[i:i + 1], i)
        o = om.forward(oc, ids[i:i + 1], i)
        check_logits(a, o, dtype, "split-S decode step %d" % i)
        np.testing.assert_allclose(a, b, atol=1e-4 if dtype == "f32" else 5e-2, rtol=0)


@pytest.mark.parametrize("name", ["llama_a", "mistral_a", "qwen2_a"])
@needs_experimental
def test_fused_attention_oproj_launch(fa, name, monkeypatch):
    """FL_FUSE_OPROJ=1: decode attention + o_proj in one launch (W_o cut along K by kv head, slice in LDS, one word per
    kv head, bounded poll, partial vectors summed by the next norm prologue) must give the two-launch result, also
    across many steps of one decode call and with split S."""
    cfg = synth.CONFIGS[name]
    w = synth.synth_weights(cfg)
    ids = synth.prompt_ids(cfg, 12, seed=9)
    ref = fa.Model(cfg, w, dtype="bf16")
    rc = ref.new_cache(600)
    ref.forward(rc, ids[:10], 0)
    want = [ref.forward(rc, ids[i:i + 1], i) for i in (10, 11)]
    tok = oracle.argmax(want[-1])
    want_toks = ref.decode_greedy(rc, tok, 12, 20)
    monkeypatch.setenv("FL_FUSE_OPROJ", "1")
    m = fa.Model(cfg, w, dtype="bf16")
    c = m.new_cache(600)                       # 600 positions -> 5 attention splits of 128
    m.forward(c, ids[:10], 0)
    for i, wnt in zip((10, 11), want):
        check_logits(m.forward(c, ids[i:i + 1], i), wnt, "bf16", "fused attn+oproj step %d" % i)
    got_toks = m.decode_greedy(c, tok, 12, 20)
    assert len(got_toks) == 20
    same = int(np.argmin(np.concatenate([got_toks == want_toks, [False]])))
    assert same >= 10, (got_toks, want_toks)   # bf16 split-order noise may fork the two greedy runs late


@needs_experimental
@pytest.mark.parametrize("cap", [600, 768, 1000])
def test_fused_attention_oproj_mistral_width(fa, cap, monkeypatch):
    """The fused launch (opt-in) at Mistral-7B's layer shape (8 kv heads: one group of 32 workgroups per head, ~150 rows
    of W_o per workgroup in LDS).  FL_FUSE_OPROJ=-1 (the rule "where it pays most"): 600 positions = 5 splits, attention
    workgroups without rows; 768 = 6 splits, 7 rows each; FL_FUSE_OPROJ=1 (wherever it fits): 1000 = 8 splits, 44 rows
    each.  Against the two-launch path after a 300-token prefill, step by step and as one greedy decode call."""
    cfg = synth.CONFIGS["mistral_wide"]
    w = synth.synth_weights(cfg)
    ids = synth.prompt_ids(cfg, 306, seed=21)
    monkeypatch.setenv("FL_FUSE_OPROJ", "0")
    ref = fa.Model(cfg, w, dtype="bf16")
    rc = ref.new_cache(cap)
    ref.forward(rc, ids[:300], 0)
    want = [ref.forward(rc, ids[i:i + 1], i) for i in range(300, 306)]
    tok = oracle.argmax(want[-1])
    want_toks = ref.decode_greedy(rc, tok, 306, 24)
    monkeypatch.setenv("FL_FUSE_OPROJ", "1" if cap > 768 else "-1")
    m = fa.Model(cfg, w, dtype="bf16")
    c = m.new_cache(cap)
    m.forward(c, ids[:300], 0)
    for i, wnt in zip(range(300, 306), want):
        got = m.forward(c, ids[i:i + 1], i)
        rel = np.linalg.norm(got - wnt) / np.linalg.norm(wnt)
        assert rel < 1e-2, (i, rel)            # bf16 noise between two summation orders of o_proj (measured ~2e-3)
        assert int(np.argmax(got)) == int(np.argmax(wnt))
    got_toks = m.decode_greedy(c, tok, 306, 24)
    assert len(got_toks) == 24
    same = int(np.argmin(np.concatenate([got_toks == want_toks, [False]])))
    assert same >= 8, (got_toks, want_toks)    # bf16 split-order noise may fork the two greedy runs late
    # the hand-offs inside the launch leave no run-to-run freedom: the same state decodes to the same ids, bit for bit
    # (a partial read before its split was published would show here)
    if cap == 768:
        runs = []
        for _ in range(3):
            c2 = m.new_cache(cap)
            m.forward(c2, ids[:300], 0)
            runs.append(m.decode_greedy(c2, int(ids[300]), 300, 200))
            c2.close()
        np.testing.assert_array_equal(runs[0], runs[1])
        np.testing.assert_array_equal(runs[0], runs[2])
    # ... and it IS the fused launch that ran
    m.profile_begin()
    m.forward(c, ids[5:6], 330)
    names = [k["name"] for k in m.profile_end()]
    assert any("oproj" in n for n in names), names


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_chunked_prefill_and_prefix(fa, case, dtype, monkeypatch):
    """Two T>1 calls (the second sees a cached prefix: keys < len are visible whatever the window, App. A.5)
    and a prefill that the library itself cuts into chunks (FL_PREFILL_CHUNK) must match one oracle prefill
    per API call: library chunking keeps the single call's causal + sliding-window mask."""
    name, cfg, w = case
    gm, om = _models(fa, cfg, w, dtype)
    ids = synth.prompt_ids(cfg, 30, seed=12)
    gc, oc = gm.new_cache(64), om.new_cache(64)
    check_logits(gm.forward(gc, ids[:11], 0), om.forward(oc, ids[:11], 0), dtype, "first chunk")
    check_logits(gm.forward(gc, ids[11:30], 11), om.forward(oc, ids[11:30], 11), dtype, "second chunk over a prefix")
    assert len(gc) == 30
    monkeypatch.setenv("FL_PREFILL_CHUNK", "7")            # 30 tokens -> 7+7+7+7+2; also a 1-token tail for 29
    g2 = fa.Model(cfg, w, dtype=dtype)
    o2 = om.new_cache(64)
    c2 = g2.new_cache(64)
    check_logits(g2.forward(c2, ids[:29], 0), om.forward(o2, ids[:29], 0), dtype, "library-chunked prefill")
    # ... and over a cached prefix: 8 cached, then 22 = 7+7+6+2 (no 1-token tail chunk is ever cut)
    c3, o3 = g2.new_cache(64), om.new_cache(64)
    g2.forward(c3, ids[:8], 0); om.forward(o3, ids[:8], 0)
    check_logits(g2.forward(c3, ids[8:30], 8), om.forward(o3, ids[8:30], 8), dtype, "library-chunked prefill over a prefix")


def test_f16_and_f32_source_tensors(fa):
    """initialize_model casts whatever dtype the checkpoint holds (VarBuilder::from_tensors): f16 / f32 / bf16
    sources of the same values give the same model."""
    cfg = synth.CONFIGS["llama_a"]
    wb = synth.synth_weights(cfg)
    wf = synth.as_f32(wb)
    # values exactly representable in f16 as well: quantise the bf16 values to f16 and back first
    w16 = {k: v.astype(np.float16) for k, v in wf.items()}
    wf16 = {k: v.astype(np.float32) for k, v in w16.items()}
    ids = synth.prompt_ids(cfg, 9)
    a = fa.Model(cfg, w16, dtype="f32")
    b = fa.Model(cfg, wf16, dtype="f32")
    ca, cb = a.new_cache(16), b.new_cache(16)
    np.testing.assert_array_equal(a.forward(ca, ids, 0), b.forward(cb, ids, 0))
    c = fa.Model(cfg, wb, dtype="f32")
    d = fa.Model(cfg, wf, dtype="f32")
    cc, cd = c.new_cache(16), d.new_cache(16)
    np.testing.assert_array_equal(c.forward(cc, ids, 0), d.forward(cd, ids, 0))
    # ... and sources the bf16 build has to ROUND (fp32 values that are no bf16 values; f16 values with more significand bits than
    # bf16 keeps) give the model of the rounded values handed in as bf16: the build's conversion is model_image_ref.convert
    import model_image_ref as ref
    for src_dtype in ("f32", "f16"):
        src = ref.rounding_sources(wb, src_dtype, "model.layers.0.self_attn.q_proj.weight", special_row=False)
        rounded = {k: ref.convert(v, src_dtype, "bf16") for k, v in src.items()}
        assert any(not np.array_equal(rounded[k], wb[k]) for k in wb)
        e, f = fa.Model(cfg, src, dtype="bf16"), fa.Model(cfg, rounded, dtype="bf16")
        ce, cf = e.new_cache(16), f.new_cache(16)
        le, lf = e.forward(ce, ids, 0), f.forward(cf, ids, 0)
        assert np.isfinite(le).all()
        np.testing.assert_array_equal(le, lf)                                     # prefill
        tok = int(np.argmax(le))
        np.testing.assert_array_equal(e.forward(ce, [tok], len(ids)), f.forward(cf, [tok], len(ids)))       # a decode step


def test_concurrent_streams_on_one_model(fa):
    """The reference's streaming path runs several generations on clones of one model concurrently
    (mod.rs:137-238).  Distinct caches on one fl_model from several threads must not interfere."""
    import threading
    cfg = synth.CONFIGS["mistral_a"]
    w = synth.synth_weights(cfg)
    gm = fa.Model(cfg, w, dtype="bf16")
    prompts = [synth.prompt_ids(cfg, 6 + k, seed=100 + k) for k in range(6)]

    def run(p):
        c = gm.new_cache(64)
        first = gm.forward_argmax(c, p, 0)
        return np.concatenate([[first], gm.decode_greedy(c, first, len(p), 12)])
    want = [run(p) for p in prompts]
    got = [None] * len(prompts)

    def worker(k):
        got[k] = run(prompts[k])
    ts = [threading.Thread(target=worker, args=(k,)) for k in range(len(prompts))]
    [t.start() for t in ts]
    [t.join() for t in ts]
    for a, b in zip(got, want):
        np.testing.assert_array_equal(a, b)


def test_long_decode_keeps_matching_the_oracle(fa):
    """64 teacher-forced decode steps through the captured graph: no drift, no state leak between replays."""
    cfg = synth.CONFIGS["qwen2_a"]
    w = synth.synth_weights(cfg)
    gm, om = _models(fa, cfg, w, "f32")
    ids = synth.prompt_ids(cfg, 80, seed=31)
    gc, oc = gm.new_cache(96), om.new_cache(96)
    gm.forward(gc, ids[:16], 0); om.forward(oc, ids[:16], 0)
    for i in range(16, 80):
        np.testing.assert_allclose(gm.forward(gc, ids[i:i + 1], i), om.forward(oc, ids[i:i + 1], i), atol=FP32_TOL, rtol=0)
