"""The verify step (fl_forward_verify) and the cache rollback (fl_cache_truncate) on the GPU.

  1. what comes back is what numpy derives from the returned logits and the draft; every row is the oracle's teacher-forced ONE-token
     forward (bf16 / fp32 bars of the parity tests); the last row is fl_forward's on the same ids (different kernels, same data:
     the `tight` bar of test_gpu_batch.py, 1e-2 relative L2); the cache grows by what was returned;
  2. rejected rows leave no trace: two calls that differ only behind the first wrong id agree bit for bit, now and later;
  3. fl_cache_truncate: a rolled-back cache is the cache that never went there -- also after graph replays and inside a batch;
  4. ties take the LAST maximal index on every row;
  5. the sliding-window and tensor-parallel refusals."""
import numpy as np
import pytest

import synth
from oracle import oracle
from test_gpu_parity import check_logits

pytestmark = pytest.mark.gpu

MODELS = ["llama_a", "mistral_a", "qwen2_a", "llama_mha", "llama_d100"]
CAP = 96


@pytest.fixture(scope="module")
def fa():
    import fastllm_amd
    assert fastllm_amd.device_count() >= 1
    return fastllm_amd


_models = {}


def models(fa, name, dtype):
    """(GPU model, oracle, weights) of a config, built once per module."""
    key = (name, dtype)
    if key not in _models:
        cfg = synth.CONFIGS[name]
        w = synth.synth_weights(cfg)
        _models[key] = (fa.Model(cfg, w, dtype=dtype), oracle.OracleModel(cfg, synth.as_f32(w), round_bf16=(dtype == "bf16")), w)
    return _models[key]


def argmax_last(row):
    return int(row.size - 1 - np.argmax(row[::-1]))


def expected(lg, draft):
    """numpy on the returned logits: the ids the call must hand back."""
    a = [argmax_last(r) for r in lg]
    n = 0
    while n < len(draft) and int(draft[n]) == a[n]:
        n += 1
    return a[: n + 1]


def prefill(gm, cfg, L, seed=1234):
    p = synth.prompt_ids(cfg, L, seed=seed)
    c = gm.new_cache(CAP)
    first = gm.forward_argmax(c, p, 0)
    return c, p, first


def continuation(gm, cfg, L, n, seed=1234):
    """The model's own greedy continuation of the prompt (a twin cache, the decode kernels)."""
    c, _, first = prefill(gm, cfg, L, seed)
    return first, gm.decode_greedy(c, first, L, n)


def half_right(cfg, cont, n_draft):
    """The true continuation with a wrong id in the middle (n_draft >= 7): accepted rows, a rejection and rows behind it in one call."""
    d = np.array(cont[:n_draft], np.uint32)
    if n_draft >= 7:
        d[n_draft // 2] = (d[n_draft // 2] + 1) % cfg["vocab_size"]
    return d


def check_step(fa, name, dtype, L, n_draft, draft_of=half_right):
    cfg = synth.CONFIGS[name]
    gm, om, _ = models(fa, name, dtype)
    first, cont = continuation(gm, cfg, L, 15)
    draft = draft_of(cfg, cont, n_draft)
    c, p, first2 = prefill(gm, cfg, L)
    assert first2 == first
    toks, lg = gm.forward_verify(c, first, draft, L, want_logits=True)
    assert lg.shape == (n_draft + 1, cfg["vocab_size"])
    assert toks.tolist() == expected(lg, draft), (name, dtype, L, n_draft)
    assert len(c) == L + len(toks)
    # every row: the oracle teacher-forced with one-token forwards of the same ids
    oc = om.new_cache(CAP)
    om.forward(oc, p, 0)
    ids = [first] + draft.tolist()
    for t, tok in enumerate(ids):
        check_logits(lg[t], om.forward(oc, [tok], L + t), dtype, "%s %s L %d n_draft %d row %d" % (name, dtype, L, n_draft, t))
    # the last row: fl_forward of the same ids on a twin cache
    twin, _, _ = prefill(gm, cfg, L)
    ref = gm.forward(twin, ids, L)
    rel = np.linalg.norm(lg[-1] - ref) / np.linalg.norm(ref)
    print("%s %s L %d n_draft %d: last row vs fl_forward rel L2 %.3e, %d of %d accepted" % (name, dtype, L, n_draft, rel, len(toks) - 1, n_draft))
    assert rel <= 1e-2, rel
    return toks


@pytest.mark.parametrize("n_draft", [0, 1, 7, 15])
@pytest.mark.parametrize("L", [5, 37])
@pytest.mark.parametrize("dtype", ["bf16", "f32"])
@pytest.mark.parametrize("name", MODELS)
def test_verify_step(fa, name, dtype, L, n_draft):
    toks = check_step(fa, name, dtype, L, n_draft)
    if dtype == "f32" and n_draft >= 7:
        assert len(toks) == n_draft // 2 + 1            # fp32: the rows ARE the decode steps' -- accepted up to the planted wrong id


@pytest.mark.parametrize("j", [0, 3, 14])
@pytest.mark.parametrize("dtype", ["bf16", "f32"])
@pytest.mark.parametrize("name", ["llama_a", "mistral_a", "qwen2_a"])
def test_rejected_rows_leave_no_trace(fa, name, dtype, j):
    cfg = synth.CONFIGS[name]
    V = cfg["vocab_size"]
    gm, _, _ = models(fa, name, dtype)
    L = 37
    first, cont = continuation(gm, cfg, L, 15)
    da = np.array(cont, np.uint32)
    da[j] = (da[j] + 1) % V                                             # the wrong id; what follows it is the true continuation in A ...
    db = da.copy()
    db[j + 1:] = (db[j + 1:] + 7 + np.arange(14 - j)) % V               # ... and something else in B
    outs = []
    for d in (da, db):
        c, _, _ = prefill(gm, cfg, L)
        toks, lg = gm.forward_verify(c, first, d, L, want_logits=True)
        assert len(c) == L + len(toks)
        tok, pos, later = int(toks[-1]), L + len(toks), []
        for _ in range(4):
            x = gm.forward(c, [tok], pos)
            later.append(x)
            tok, pos = argmax_last(x), pos + 1
        outs.append((toks, lg, later))
    (ta, la, fa_), (tb, lb, fb_) = outs
    assert len(ta) <= j + 1                                             # the wrong id was not accepted
    assert np.array_equal(ta, tb)
    assert np.array_equal(la[: j + 1], lb[: j + 1])                     # bit-identical rows up to the wrong id
    if j < 14:
        assert not np.array_equal(la[j + 2:], lb[j + 2:])               # (the rows behind it did differ)
    for x, y in zip(fa_, fb_):
        assert np.array_equal(x, y)


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
@pytest.mark.parametrize("name", ["llama_a", "mistral_a", "qwen2_a", "llama_mha"])
def test_cache_truncate(fa, name, dtype):
    cfg = synth.CONFIGS[name]
    gm, _, _ = models(fa, name, dtype)
    p = synth.prompt_ids(cfg, 7)
    x = synth.prompt_ids(cfg, 6, seed=77)[1:]
    y = synth.prompt_ids(cfg, 6, seed=78)[1:]

    def base():
        c = gm.new_cache(CAP)
        gm.forward(c, p, 0)
        return c

    b = base()
    want = gm.forward(b, y, 7)
    want_dec = gm.decode_greedy(b, argmax_last(want), 12, 6)
    assert len(b) == 18

    def same_as_b(c, what):
        assert len(c) == 7
        got = gm.forward(c, y, 7)
        assert np.array_equal(got, want), what
        assert np.array_equal(gm.decode_greedy(c, argmax_last(got), 12, 6), want_dec), what
        assert len(c) == 18

    a = base()
    gm.forward(a, x, 7)
    assert len(a) == 12
    a.truncate(12)                                                      # to the current length: nothing happens
    assert len(a) == 12
    with pytest.raises(fa.FastLLMError) as e:
        a.truncate(13)
    assert e.value.code == -8 and len(a) == 12
    a.truncate(7)
    same_as_b(a, "prompt rows rolled back")
    # ... a cache that has already replayed its decode graph
    g = base()
    gm.decode_greedy(g, int(x[0]), 7, 3)
    assert len(g) == 10
    g.truncate(7)
    same_as_b(g, "decode steps rolled back")
    # ... a verify step rolled back
    v = base()
    gm.forward_verify(v, int(x[0]), x[1:], 7)
    v.truncate(7)
    same_as_b(v, "verify step rolled back")
    # truncate(0) is reset
    a.truncate(0)
    assert len(a) == 0
    fresh = gm.new_cache(CAP)
    assert np.array_equal(gm.forward(a, p, 0), gm.forward(fresh, p, 0))
    same_as_b(a, "after truncate(0)")


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_cache_truncate_on_a_batch_member(fa, dtype):
    name = "mistral_a"
    cfg = synth.CONFIGS[name]
    gm, _, _ = models(fa, name, dtype)
    lens = [7, 11]

    def members():
        cs = []
        for i, n in enumerate(lens):
            c = gm.new_cache(CAP)
            gm.forward(c, synth.prompt_ids(cfg, n, seed=60 + i), 0)
            cs.append(c)
        return cs

    ca, cb = members(), members()
    ba, bb = fa.Batch(gm, ca), fa.Batch(gm, cb)
    t1, t2 = [3, 4], [9, 10]
    ba.forward(t1, lens)
    assert [len(c) for c in ca] == [8, 12]
    ca[0].truncate(7)                                                    # both members back, between two batch.forward calls
    ca[1].truncate(11)
    lg_a, am_a = ba.forward(t2, lens)
    lg_b, am_b = bb.forward(t2, lens)                                    # the twin batch never saw t1
    assert np.array_equal(lg_a, lg_b) and np.array_equal(am_a, am_b)
    assert [len(c) for c in ca] == [len(c) for c in cb] == [8, 12]
    # one member back, the other goes on: each row is its own sequence's
    ca[0].truncate(7)
    cb[0].truncate(7)
    lg_a, _ = ba.forward([t1[0], 5], [7, 12])
    lg_b, _ = bb.forward([t1[0], 5], [7, 12])
    assert np.array_equal(lg_a, lg_b)
    for b in (ba, bb):
        b.close()


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_ties_take_the_last_index_on_every_row(fa, dtype):
    name = "llama_a"
    cfg = synth.CONFIGS[name]
    V = cfg["vocab_size"]
    gm, _, w = models(fa, name, dtype)
    L, nd = 5, 7
    first, cont = continuation(gm, cfg, L, nd + 1)
    c, _, _ = prefill(gm, cfg, L)
    toks, _ = gm.forward_verify(c, first, cont[:nd], L)
    a = toks.tolist()                                                    # a[t]: the ArgMax of row t (as far as the rows were accepted)
    t = next(t for t in range(1, len(a)) if a[t] not in a[:t] and a[t] < V - 1)
    r = a[t]
    r2 = max(i for i in range(r + 1, V) if i not in a and i != first)
    w2 = dict(w)
    lm = w["lm_head.weight"].copy()
    lm[r2] = lm[r]                                                       # lm_head rows r < r2 are copies: wherever r wins, r2 ties
    w2["lm_head.weight"] = lm
    gm2 = fa.Model(cfg, w2, dtype=dtype)
    c2 = gm2.new_cache(CAP)
    assert gm2.forward_argmax(c2, synth.prompt_ids(cfg, L), 0) == first
    toks2, lg2 = gm2.forward_verify(c2, first, cont[:nd], L, want_logits=True)
    assert lg2[t, r] == lg2[t, r2] == lg2[t].max()                       # the tie is there, bit for bit
    assert toks2.tolist() == a[:t] + [r2]                                # rows before it as before; row t takes the LAST maximal index
    gm2.close()


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
@pytest.mark.parametrize("name", ["mistral_win", "qwen2_win"])
def test_window(fa, name, dtype):
    """sliding_window 5: n_draft = 5 still equals successive (unmasked) decode steps; 6 would hide the first new key from the last row."""
    for L in (5, 37):
        check_step(fa, name, dtype, L, 5, draft_of=lambda cfg, cont, n: np.array(cont[:n], np.uint32))
    gm, _, _ = models(fa, name, dtype)
    cfg = synth.CONFIGS[name]
    c, _, first = prefill(gm, cfg, 5)
    with pytest.raises(fa.FastLLMError) as e:
        gm.forward_verify(c, first, [1] * 6, 5)
    assert e.value.code == -10 and "sliding_window" in str(e.value) and len(c) == 5


def test_tensor_parallel_is_refused(fa):
    cfg = synth.CONFIGS["llama_a"]
    gm = fa.Model(cfg, synth.synth_weights(cfg), dtype="bf16", tp_mode=fa.binding.TP_EMULATED, tp_size=2)
    c = gm.new_cache(CAP)
    first = gm.forward_argmax(c, synth.prompt_ids(cfg, 5), 0)
    with pytest.raises(fa.FastLLMError) as e:
        gm.forward_verify(c, first, [1, 2], 5)
    assert e.value.code == -10 and len(c) == 5
    with pytest.raises(fa.FastLLMError) as e:
        gm.decode_lookup(c, [1, 2, 3], first, 5, 8)
    assert e.value.code == -10 and len(c) == 5
    gm.close()
