"""Speculative decode for sampled requests through the C ABI (fl_forward_verify_ex, fl_decode_lookup_ex).

Correctness of a step is defined on the rows it returns (logits_out), so no numeric margin is involved: the token of row i is
topp_checker.Checker's draw with word draws_done + i, the accepted count is the scan of the draft against the tokens, the cache grows by
what was returned.  Only the tc.MARGIN excuse of the sampler tests applies (a draw within 1e-6 of a boundary of its cumulative interval).

  1. steps: starting from the one-row sampled continuation (and, to see a rejection at every position whatever the dtype, from a draft
     that is wrong everywhere), the draft is corrected by what each call returns; rows up to the first wrong id are bit-identical
     between such calls (test_gpu_verify.py), so the accepted count grows by at least one per call and reaches n_draft;
  2. rejected rows leave no trace;
  3. the loop: fl_decode_lookup_ex equals, id for id and in its stats, a Python loop of lookup_draft + forward_verify(draws_done = 1 +
     emitted) -- the word accounting across steps; max_draft = 0 is decode_sample; top_k = 1 forces acceptance and gives decode_greedy;
  4. EOS inside an accepted run, the room, the refusals, the host mirror."""
import ctypes as C

import numpy as np
import pytest

import synth
import topp_checker as tc
from oracle import oracle
from test_gpu_decode_lookup import CAP, L as LP, N, SEEDS, corpora, simulate
from test_gpu_host_mirror import generate, make  # noqa: F401
from test_host_mirror import host  # noqa: F401

pytestmark = pytest.mark.gpu

SP = dict(temperature=0.8, top_p=0.9, top_k=None, seed=7)
SP_ALL = dict(temperature=1.0, top_p=None, top_k=None, seed=3)


@pytest.fixture(scope="module")
def fa():
    import fastllm_amd
    assert fastllm_amd.device_count() >= 1
    return fastllm_amd


_models = {}
_excused = set()


def model(fa, name, dtype, **kw):
    key = (name, dtype, tuple(sorted(kw.items())))
    if key not in _models:
        cfg = synth.CONFIGS[name]
        _models[key] = fa.Model(cfg, synth.synth_weights(cfg), dtype=dtype, **kw)
    return _models[key]


def word(seed, index):
    o = oracle.Sampler(seed, 1.0)
    o._s.rng.word = index
    return o.next_u32()


def kw(sp, draws_done):
    return dict(temperature=sp["temperature"], top_p=sp["top_p"], top_k=sp["top_k"], seed=sp["seed"], draws_done=draws_done)


def prefill(gm, cfg, L, sp, seed=1234, cap=CAP):
    """a cache holding the prompt, and the prompt's own token drawn with word 0"""
    p = synth.prompt_ids(cfg, L, seed=seed)
    c = gm.new_cache(cap)
    return c, p, gm.forward_sample(c, p, 0, sp["temperature"], seed=sp["seed"], draws_done=0, top_p=sp["top_p"], top_k=sp["top_k"])


def verify_checked(gm, c, token, draft, pos, sp, w0, case):
    """One sampled verify call, checked on its own rows.  Returns (tokens, logits)."""
    draft = np.asarray(draft, np.uint32)
    len0 = len(c)
    toks, lg = gm.forward_verify(c, token, draft, pos, want_logits=True, **kw(sp, w0))
    n_acc = len(toks) - 1
    assert lg.shape[0] == draft.size + 1 and 0 <= n_acc <= draft.size
    assert len(c) == len0 + n_acc + 1, case
    for i in range(n_acc + 1):                            # every returned token: the checker's draw from row i with word w0 + i
        tok, near = tc.Checker(tc.prs_of(lg[i], sp["temperature"]), sp["top_p"], sp["top_k"]).draw(word(sp["seed"], w0 + i))
        if tok != int(toks[i]):
            assert near <= tc.MARGIN, "%s row %d: device %d checker %d, %.3g from a boundary" % (case, i, int(toks[i]), tok, near)
            _excused.add(case)
            assert len(_excused) <= 1, "more than one case needs the boundary excuse: %s" % sorted(_excused)
    # the scan: accepted while the draws equal the drafts, and not one further
    assert np.array_equal(toks[:n_acc], draft[:n_acc]), case
    assert n_acc == draft.size or toks[n_acc] != draft[n_acc], case
    return toks, lg


def continuation(gm, cfg, L, n, sp):
    """the plain sampled loop on a twin cache: the prompt's token (word 0) and n more (words 1 .. n)"""
    c, _, first = prefill(gm, cfg, L, sp)
    return first, gm.decode_sample(c, first, L, n, sp["temperature"], seed=sp["seed"], draws_done=1, top_p=sp["top_p"], top_k=sp["top_k"])


@pytest.mark.parametrize("n_draft", [1, 7, 15])
@pytest.mark.parametrize("L", [5, 12])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("name", ["llama_a", "mistral_a", "qwen2_a"])
def test_verify_steps(fa, name, dtype, L, n_draft):
    cfg = synth.CONFIGS[name]
    V = cfg["vocab_size"]
    gm = model(fa, name, dtype)
    for sp in (SP, SP_ALL):
        first, cont = continuation(gm, cfg, L, n_draft, sp)
        assert len(cont) == n_draft
        for start in ("continuation", "all wrong"):
            case = "%s %s L %d n_draft %d t %g %s" % (name, dtype, L, n_draft, sp["temperature"], start)
            draft = np.array(cont, np.uint32) if start == "continuation" else (np.array(cont, np.uint32) + 1) % V
            n_prev, calls, prev_lg = -1, 0, None
            while True:
                c, _, f = prefill(gm, cfg, L, sp)
                assert f == first
                toks, lg = verify_checked(gm, c, first, draft, L, sp, 1, case)
                calls += 1
                n_acc = len(toks) - 1
                if prev_lg is not None:                   # rows up to the first wrong id of the call before: bit for bit
                    assert np.array_equal(lg[: n_prev + 1], prev_lg[: n_prev + 1]), case
                assert n_acc >= min(n_prev + 1, n_draft), (case, n_prev, n_acc)
                if start == "all wrong" and calls == 1:
                    assert n_acc == 0
                if n_acc == n_draft:
                    break
                draft[: n_acc + 1] = toks                 # the accepted ids (unchanged) and the model's own draw at the rejection
                n_prev, prev_lg = n_acc, lg
                assert calls <= n_draft, case
            assert calls <= n_draft + 1
            if dtype == "f32" and start == "continuation":
                # fp32 rows are the decode steps' up to the last bits: the plain loop's tokens come back (boundary draws excepted)
                print("%s: %d call(s)" % (case, calls))


@pytest.mark.parametrize("j", [0, 3, 14])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("name", ["llama_a", "mistral_a", "qwen2_a"])
def test_rejected_rows_leave_no_trace(fa, name, dtype, j):
    cfg = synth.CONFIGS[name]
    V = cfg["vocab_size"]
    gm = model(fa, name, dtype)
    L, sp = 12, SP
    case = "%s %s no trace j %d" % (name, dtype, j)
    first, cont = continuation(gm, cfg, L, 15, sp)
    # a draft the call itself confirms up to j: corrected call by call as in test_verify_steps, then made wrong at j
    draft = np.array(cont, np.uint32)
    for _ in range(16):
        c, _, _ = prefill(gm, cfg, L, sp)
        toks, _ = verify_checked(gm, c, first, draft, L, sp, 1, case)
        if len(toks) - 1 >= min(j + 1, 15):
            break
        draft[: len(toks)] = toks
    da = draft.copy()
    da[j] = (da[j] + 1) % V
    db = da.copy()
    db[j + 1:] = (db[j + 1:] + 7 + np.arange(14 - j)) % V
    outs = []
    for d in (da, db):
        c, _, _ = prefill(gm, cfg, L, sp)
        toks, lg = verify_checked(gm, c, first, d, L, sp, 1, case)
        assert len(toks) == j + 1 and len(c) == L + j + 1
        nxt = gm.forward_sample(c, [int(toks[-1])], L + j + 1, sp["temperature"], seed=sp["seed"], draws_done=1 + j + 1, top_p=sp["top_p"])
        later = gm.forward(c, [nxt], L + j + 2)
        outs.append((toks, lg, nxt, later))
    (ta, la, na, fa_), (tb, lb, nb, fb_) = outs
    assert np.array_equal(ta, tb) and np.array_equal(la[: j + 1], lb[: j + 1]) and na == nb and np.array_equal(fa_, fb_)
    # a twin that took the accepted tokens one by one: the one-row sampled step behind them draws the same token
    t, _, f = prefill(gm, cfg, L, sp)
    ids = [f] + ta[:-1].tolist()
    for s, tok in enumerate(ids):
        got = gm.forward_sample(t, [tok], L + s, sp["temperature"], seed=sp["seed"], draws_done=1 + s, top_p=sp["top_p"])
        if dtype == "f32":
            assert got == int(ta[s]), (case, s)           # ... as every step before it drew the call's tokens
    assert len(t) == L + j + 1
    nt = gm.forward_sample(t, [int(ta[-1])], L + j + 1, sp["temperature"], seed=sp["seed"], draws_done=1 + j + 1, top_p=sp["top_p"])
    if dtype == "f32":
        assert nt == na, case


def start(gm, name, sp, cap=CAP):
    return prefill(gm, synth.CONFIGS[name], LP, sp, seed=SEEDS[name], cap=cap)


def python_loop(fa, gm, c, corpus, first, pos, n_steps, sp, max_draft, ngram_max, ngram_min, case, window=None):
    """fl_decode_lookup_ex restated: lookup_draft + forward_verify with draws_done = 1 + emitted, every step checked on its rows"""
    hist = list(corpus) + [first]
    out, st, tok = [], dict(steps=0, drafted=0, accepted=0), first
    while len(out) < n_steps:
        limit = min(n_steps - len(out) - 1, c.capacity() - len(c) - 1)
        if window is not None:
            limit = min(limit, window)
        d = fa.lookup_draft(hist, limit, max_draft=max_draft, ngram_max=ngram_max, ngram_min=ngram_min)
        toks, _ = verify_checked(gm, c, tok, d, pos + len(out), sp, 1 + len(out), case)
        st["steps"] += 1
        st["drafted"] += len(d)
        st["accepted"] += len(toks) - 1
        out += toks.tolist()
        hist += toks.tolist()
        tok = int(toks[-1])
    return np.array(out, np.uint32), st


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("name", ["llama_a", "mistral_a", "qwen2_a"])
def test_loop_equals_the_python_loop(fa, name, dtype):
    cfg = synth.CONFIGS[name]
    gm = model(fa, name, dtype)
    sp = SP
    twin, p, first = start(gm, name, sp)
    plain = gm.decode_sample(twin, first, LP, N, sp["temperature"], seed=sp["seed"], draws_done=1, top_p=sp["top_p"])
    clean, bad = corpora(cfg, p, first, plain)
    n_drafted = 0
    for corpus in (clean, bad):
        for max_draft in (1, 7, 15):
            for ng in ((3, 1), (2, 2)):
                case = "%s %s loop max_draft %d ngram %s" % (name, dtype, max_draft, ng)
                c, _, f = start(gm, name, sp)
                got, st = gm.decode_lookup(c, corpus, f, LP, N, max_draft=max_draft, ngram_max=ng[0], ngram_min=ng[1], return_stats=True, **kw(sp, 1))
                c2, _, _ = start(gm, name, sp)
                want, st2 = python_loop(fa, gm, c2, corpus, f, LP, N, sp, max_draft, ng[0], ng[1], case)
                assert np.array_equal(got, want) and st == st2, (case, st, st2)
                assert len(c) == len(c2) == LP + N
                n_drafted += st["drafted"]
                if dtype == "f32":
                    assert np.array_equal(got, plain), case       # ... and the plain loop's seeded stream (no boundary draw among these)
    assert n_drafted > 0


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("name", ["llama_a", "mistral_a", "qwen2_a"])
def test_loop_with_drafting_off_is_decode_sample(fa, name, dtype):
    gm = model(fa, name, dtype)
    for sp in (SP, SP_ALL):
        twin, p, first = start(gm, name, sp)
        want = gm.decode_sample(twin, first, LP, N, sp["temperature"], seed=sp["seed"], draws_done=1, top_p=sp["top_p"], top_k=sp["top_k"])
        c, _, f = start(gm, name, sp)
        got, st = gm.decode_lookup(c, p, f, LP, N, max_draft=0, return_stats=True, **kw(sp, 1))
        assert f == first and np.array_equal(got, want) and st == dict(steps=N, drafted=0, accepted=0) and len(c) == len(twin) == LP + N


def same_or_near_tie(gm, name, got, want, case):
    """bf16: only a near-tie of the two largest logits may separate the two paths (test_gpu_decode_lookup.py's rule and number)."""
    assert len(got) == len(want)
    if np.array_equal(got, want):
        return
    k = int(np.argmax(got != want))
    p = synth.prompt_ids(synth.CONFIGS[name], LP, seed=SEEDS[name])
    c = gm.new_cache(CAP)
    first = gm.forward_argmax(c, p, 0)
    lg = None
    for s, t in enumerate([first] + want[:k].tolist()):
        lg = gm.forward(c, [t], LP + s)
    top2 = np.sort(lg)[-2:]
    print("%s: differs from decode_greedy at %d, top-two gap %.3e of %.3e" % (case, k, top2[1] - top2[0], np.abs(lg).max()))
    assert top2[1] - top2[0] < 4e-2 * max(1.0, np.abs(lg).max()), "%s diverges at %d with a clear margin" % (case, k)
    _near_ties.add(case)
    assert len(_near_ties) <= 1, "more than one bf16 case needs the near-tie excuse: %s" % sorted(_near_ties)


_near_ties = set()
TOP1 = dict(temperature=0.8, top_p=None, top_k=1, seed=11)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("name", list(SEEDS))
def test_loop_with_acceptance_forced(fa, name, dtype):
    """top_k = 1 keeps the lowest maximal index, ArgMax the last: they coincide on these prompt seeds (their fp32 top-two gap is asserted
    on the CPU in test_gpu_decode_lookup.py), so the sampled loop must return decode_greedy's tokens and the corpus forces acceptance."""
    cfg = synth.CONFIGS[name]
    gm = model(fa, name, dtype)
    p = synth.prompt_ids(cfg, LP, seed=SEEDS[name])
    twin = gm.new_cache(CAP)
    first = gm.forward_argmax(twin, p, 0)
    want = gm.decode_greedy(twin, first, LP, N)
    clean, bad = corpora(cfg, p, first, want)
    for corpus, what in ((clean, "clean"), (bad, "corrupted")):
        for ng in ((3, 1), (2, 2)):
            c = gm.new_cache(CAP)
            assert gm.forward_argmax(c, p, 0) == first
            got, st = gm.decode_lookup(c, corpus, first, LP, N, max_draft=7, ngram_max=ng[0], ngram_min=ng[1], return_stats=True, **kw(TOP1, 1))
            assert len(c) == LP + N
            if dtype == "f32":
                assert np.array_equal(got, want), (name, what, ng)
                sim, _ = simulate(corpus, first, want, 7, ng[0], ng[1])
                assert st == sim, (name, what, ng, st, sim)
            else:
                same_or_near_tie(gm, name, got, want, "bf16 top_k 1 " + name)
            if np.array_equal(got, want):
                if what == "clean":
                    assert st["accepted"] / st["steps"] >= 3 and st["steps"] < N / 3, (name, ng, st)
                else:
                    assert st["drafted"] > st["accepted"] > 0, (name, ng, st)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("name", ["llama_a", "mistral_a", "qwen2_a"])
def test_eos_inside_an_accepted_run(fa, name, dtype):
    cfg = synth.CONFIGS[name]
    gm = model(fa, name, dtype)
    p = synth.prompt_ids(cfg, LP, seed=SEEDS[name])

    def begin():
        c = gm.new_cache(CAP)
        return c, gm.forward_argmax(c, p, 0)

    twin, first = begin()
    want = gm.decode_greedy(twin, first, LP, N)
    clean, _ = corpora(cfg, p, first, want)
    _, starts = simulate(clean, first, want, 7, 3, 1)
    ends = starts[1:] + [N]
    i = next(i for s, e in zip(starts, ends) for i in range(s + 1, e - 1) if want[i] not in want[:i] and want[i] != first)
    eos = int(want[i])
    c, f = begin()
    got = gm.decode_lookup(c, clean, f, LP, N, eos=eos, **kw(TOP1, 1))
    t2, _ = begin()
    plain = gm.decode_sample(t2, first, LP, N, TOP1["temperature"], seed=TOP1["seed"], draws_done=1, eos=eos, top_k=1)
    if dtype == "f32":
        assert np.array_equal(got, want[:i]) and np.array_equal(plain, want[:i])
    assert len(c) == LP + len(got) + (1 if len(got) < N else 0)          # the EOS's own forward is cached, nothing behind it
    if np.array_equal(got, plain):
        assert len(c) == len(t2)                                         # ... the length the plain sampled loop leaves
    # with a real sampler: the loop stops where the plain sampled loop stops, having consumed the same words
    sp = SP
    tw, _, fs = start(gm, name, sp)
    full = gm.decode_sample(tw, fs, LP, N, sp["temperature"], seed=sp["seed"], draws_done=1, top_p=sp["top_p"])
    k = next((k for k in range(2, N) if full[k] not in full[:k] and full[k] != fs), None)
    if k is not None and dtype == "f32":
        clean_s, _ = corpora(cfg, p, fs, full)
        c3, _, _ = start(gm, name, sp)
        got = gm.decode_lookup(c3, clean_s, fs, LP, N, eos=int(full[k]), **kw(sp, 1))
        assert np.array_equal(got, full[:k]) and len(c3) == LP + k + 1
        # going on from there with word 1 + k + 1: the plain loop's next tokens
        more = gm.decode_sample(c3, int(full[k]), LP + k + 1, 4, sp["temperature"], seed=sp["seed"], draws_done=1 + k + 1, top_p=sp["top_p"])
        assert np.array_equal(more, full[k + 1:k + 5])


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_room(fa, dtype):
    name, sp = "mistral_a", SP
    cfg = synth.CONFIGS[name]
    gm = model(fa, name, dtype)
    twin, p, first = start(gm, name, sp)
    want = gm.decode_sample(twin, first, LP, N, sp["temperature"], seed=sp["seed"], draws_done=1, top_p=sp["top_p"])
    clean, _ = corpora(cfg, p, first, want)
    c, _, f = start(gm, name, sp, cap=LP + N)                            # exactly the room fl_decode_sample_ex needs
    got = gm.decode_lookup(c, clean, f, LP, N, max_draft=15, **kw(sp, 1))
    assert len(got) == N and len(c) == LP + N == c.capacity()
    if dtype == "f32":
        assert np.array_equal(got, want)
    c, _, f = start(gm, name, sp, cap=LP + N - 1)
    with pytest.raises(fa.FastLLMError) as e:
        gm.decode_lookup(c, clean, f, LP, N, **kw(sp, 1))
    assert e.value.code == -7 and len(c) == LP                           # FL_ERR_SEQ_OVERFLOW before anything ran


def test_refusals(fa):
    sp = kw(SP, 1)
    cfg = synth.CONFIGS["llama_a"]
    tp = fa.Model(cfg, synth.synth_weights(cfg), dtype="bf16", tp_mode=fa.binding.TP_EMULATED, tp_size=2)
    c = tp.new_cache(CAP)
    first = tp.forward_argmax(c, synth.prompt_ids(cfg, 5), 0)
    for call in (lambda: tp.forward_verify(c, first, [1, 2], 5, **sp), lambda: tp.decode_lookup(c, [1, 2, 3], first, 5, 8, **sp)):
        with pytest.raises(fa.FastLLMError) as e:
            call()
        assert e.value.code == -10 and "tensor parallelism" in str(e.value) and len(c) == 5
    tp.close()
    # n_draft above the sliding window
    gm = model(fa, "mistral_win", "bf16")
    wcfg = synth.CONFIGS["mistral_win"]
    c = gm.new_cache(CAP)
    first = gm.forward_argmax(c, synth.prompt_ids(wcfg, 5), 0)
    toks, _ = gm.forward_verify(c, first, [1] * 5, 5, **sp)
    assert len(c) == 5 + len(toks)
    c.truncate(5)
    with pytest.raises(fa.FastLLMError) as e:
        gm.forward_verify(c, first, [1] * 6, 5, **sp)
    assert e.value.code == -10 and "sliding_window" in str(e.value) and len(c) == 5
    # a cache with logit rules or a guide
    gm = model(fa, "llama_a", "bf16")
    c = gm.new_cache(CAP)
    first = gm.forward_argmax(c, synth.prompt_ids(cfg, 5), 0)
    c.set_logit_rules(repetition_penalty=1.3)
    for call in (lambda: gm.forward_verify(c, first, [1, 2], 5, **sp), lambda: gm.decode_lookup(c, [1, 2, 3], first, 5, 8, **sp)):
        with pytest.raises(fa.FastLLMError) as e:
            call()
        assert e.value.code == -10 and len(c) == 5
    c.clear_logit_rules()
    V = cfg["vocab_size"]
    g = fa.Guide(gm, [0, V], np.arange(V, dtype=np.uint32), np.zeros(V, np.uint32))     # one state, every token allowed
    c.set_guide(g)
    for call in (lambda: gm.forward_verify(c, first, [1, 2], 5, **sp), lambda: gm.decode_lookup(c, [1, 2, 3], first, 5, 8, **sp)):
        with pytest.raises(fa.FastLLMError) as e:
            call()
        assert e.value.code == -10 and len(c) == 5
    c.clear_guide()
    toks, _ = gm.forward_verify(c, first, [1, 2], 5, **sp)              # ... and the same cache is served once they are gone
    assert len(c) == 5 + len(toks)
    # the sampler's own errors, with a model in hand
    with pytest.raises(fa.FastLLMError) as e:
        gm.forward_verify(c, first, [1, 2], len(c), temperature=0.8, top_k=-1)
    assert e.value.code == -8
    g.close()


@pytest.mark.parametrize("name", ["llama_a", "mistral_a", "qwen2_a"])
@pytest.mark.parametrize("mode", ["reference", "tokens"])
def test_host_mirror_sampled_lookup(host, name, mode, monkeypatch):
    """Model<M>::generate_ids / generate_stream_ids with SamplingOptions + LookupOptions (fp32) under top_k = 1: the ids of the plain
    request; the greedy-only overloads still refuse a temperature."""
    monkeypatch.setenv("FASTLLM_POS_MODE", mode)
    monkeypatch.setenv("FASTLLM_MAX_SEQ", "96")
    host.flh_generate_lookup.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_float, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int,
                                         C.c_void_p, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t), C.c_void_p]
    host.flh_generate_lookup_sample.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_float, C.c_int64, C.c_double, C.c_int64, C.c_int,
                                                C.c_int, C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t), C.c_void_p]
    host.flh_generate_logprobs.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_float, C.c_int64, C.c_double, C.c_int64, C.c_int,
                                           C.c_void_p, C.POINTER(C.c_size_t), C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_size_t)]
    h, cfg, _ = make(host, name, dtype=0)
    base = synth.prompt_ids(cfg, 10, seed=SEEDS[name])
    prompt = np.concatenate([base, base[1:], base[1:4]]).astype(np.uint32)       # a prompt that repeats itself: drafts from the prompt
    n = 24
    want, _ = generate(host, h, prompt, n)                                       # the host's own selection (ArgMax; top_k = 1 keeps the same id)

    def plain(temperature, top_p, top_k):
        """the device-sampled plain request (generate_ids with SamplingOptions; its log-prob form selects the same tokens)"""
        out, lp = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.float32)
        n_out, fw = C.c_size_t(0), C.c_size_t(0)
        rc = host.flh_generate_logprobs(h, prompt.ctypes.data, prompt.size, n, temperature, -1, top_p, top_k, 0, out.ctypes.data, C.byref(n_out),
                                        lp.ctypes.data, None, None, C.byref(fw))
        assert rc == 0, host.flh_last_error()
        return out[: n_out.value]

    def lookup(stream, temperature=0.8, top_p=0.0, top_k=1, eos=-1):
        out = np.zeros(n, dtype=np.uint32)
        n_out, fw = C.c_size_t(0), C.c_size_t(0)
        st = (C.c_uint64 * 3)()
        rc = host.flh_generate_lookup_sample(h, prompt.ctypes.data, prompt.size, n, temperature, eos, top_p, top_k, 7, 3, 1, stream,
                                             out.ctypes.data, C.byref(n_out), C.byref(fw), st)
        return rc, out[: n_out.value], fw.value, list(st)

    for stream in (0, 1):
        rc, got, fw, st = lookup(stream)
        assert rc == 0, host.flh_last_error()
        np.testing.assert_array_equal(got, want)
        assert fw <= n
        if not stream:
            assert fw == 1 + st[0] and st[1] >= st[2] > 0
        eos = int(want[n // 2])
        stop = int(np.flatnonzero(want == eos)[0])
        rc, got, _, _ = lookup(stream, eos=eos)
        assert rc == 0 and np.array_equal(got, want[:stop])
        # a real sampler: the ids of the plain device-sampled request with the same options
        rc, got, _, _ = lookup(stream, temperature=0.8, top_p=0.9, top_k=0)
        assert rc == 0, host.flh_last_error()
        np.testing.assert_array_equal(got, plain(0.8, 0.9, 0))
    out = np.zeros(n, dtype=np.uint32)
    n_out, fw = C.c_size_t(0), C.c_size_t(0)
    for stream in (0, 1):
        rc = host.flh_generate_lookup(h, prompt.ctypes.data, prompt.size, n, 0.8, -1, 7, 3, 1, stream, out.ctypes.data, C.byref(n_out), C.byref(fw), None)
        assert rc == -10
        if not stream:
            assert b"greedy only" in host.flh_last_error()
    host.flh_model_destroy(h)
