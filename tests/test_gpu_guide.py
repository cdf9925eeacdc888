"""Guided decoding through the model (fl_guide_create / fl_cache_set_guide: a token-level automaton masks the row every selection
reads and advances inside the device decode loop), bf16 and fp32.

Yardstick for a step: the numpy restatement of tests/guide_ref.py -- a copy of the row with -inf outside the state's list -- applied to
the row fl_forward (or fl_batch_forward) returns for the same step on a TWIN cache without a guide fed the same ids; the forward is
deterministic, so that row holds the bits the kernel read.  The state is the test's own walk.  All comparisons are exact.

The guide has three states over the model's V: state 0 allows the ids = 0 mod 3 except one banned id (the unguided run's first token)
and leads to state 1, state 1 the ids = 1 mod 3 and leads to state 2, state 2 exactly one id and leads back to state 0: the guided run
differs from the plain run at its first step, and every third token is forced."""
import ctypes as C

import numpy as np
import pytest

import guide_ref as gr
import logit_rules_ref as lr
import logprob_cases as lc
import synth
from test_host_mirror import host  # noqa: F401

pytestmark = pytest.mark.gpu
CAP = 96
NP = 8                                       # prompt length
FORCED = 5                                   # the one id of state 2
SAMPLER = dict(temperature=0.8, top_p=0.9, seed=3)
PEN = dict(repetition_penalty=1.3, frequency_penalty=0.5, presence_penalty=0.25)


@pytest.fixture(scope="module")
def fa():
    import fastllm_amd
    assert fastllm_amd.device_count() >= 1
    return fastllm_amd


@pytest.fixture(scope="module", params=["bf16", "f32"])
def env(fa, request):
    cfg = synth.CONFIGS["llama_a"]
    w = synth.synth_weights(cfg)
    return fa.Model(cfg, w, dtype=request.param), cfg, synth.prompt_ids(cfg, NP)


def automaton(V, banned):
    s0 = [i for i in range(0, V, 3) if i != int(banned)]
    return gr.Automaton([s0, np.arange(1, V, 3), [FORCED]], [1, 2, 0])


def prefilled(gm, prompt):
    c = gm.new_cache(CAP)
    return c, gm.forward_argmax(c, prompt, 0)


def setup(fa, gm, cfg, prompt):
    """The unguided greedy run, and the guide that makes the guided run differ from it at its first step."""
    c, first = prefilled(gm, prompt)
    plain = gm.decode_greedy(c, first, NP, 40)
    auto = automaton(cfg["vocab_size"], plain[0])
    return first, plain, auto, fa.Guide(gm, *auto.csr())


def guided(gm, prompt, guide, state=0):
    """A cache prefilled WITHOUT a guide (so every stream of a test starts from the same first token), then given one."""
    c, first = prefilled(gm, prompt)
    c.set_guide(guide, state)
    return c, first


def test_prefill(fa, env):
    gm, cfg, prompt = env
    a, b, c, twin = (gm.new_cache(CAP) for _ in range(4))
    plain = gm.forward_sample(a, prompt, 0, 0.0)
    auto = automaton(cfg["vocab_size"], plain)
    g = fa.Guide(gm, *auto.csr())
    row = gm.forward(twin, prompt, 0)
    for state in (0, 1, 2):
        for cache in (b, c):
            cache.reset()
            cache.set_guide(g, state)
        want = gr.argmax_last(auto.mask(row, state))
        assert gm.forward_sample(b, prompt, 0, 0.0) == want and gm.forward_argmax(c, prompt, 0) == want, state
        assert (state != 0 or want != plain) and (state != 2 or want == FORCED)
        assert b.guide_state() == c.guide_state() == auto.walk(state, want) == (state + 1) % 3
        assert len(b) == len(c) == NP
    # fl_forward on a guided cache returns the model's own row, and moves nothing
    s = b.guide_state()
    tok = int(plain)
    assert np.array_equal(gr.bits(gm.forward(b, [tok], NP)), gr.bits(gm.forward(twin, [tok], NP))) and b.guide_state() == s
    # the T == 1 forward that does select is masked in the state the cache is in
    row1 = gm.forward(twin, [tok], NP + 1)
    assert gm.forward_argmax(b, [tok], NP + 1) == gr.argmax_last(auto.mask(row1, s)) and b.guide_state() == (s + 1) % 3


def test_greedy_decode_40_steps_in_two_chunks(fa, env):
    gm, cfg, prompt = env
    V = cfg["vocab_size"]
    first, plain, auto, g = setup(fa, gm, cfg, prompt)
    free = gm.decode_greedy(guided(gm, prompt, g)[0], first, NP, 40)
    eos = next(i for i in range(V) if i not in set(free.tolist()) and i != first)      # an id that never occurs: chunks of 16 + 24
    a, _ = guided(gm, prompt, g)
    toks = gm.decode_greedy(a, first, NP, 40, eos=eos)
    assert len(toks) == 40 and np.array_equal(toks, free) and len(a) == NP + 40
    assert toks[0] != plain[0] and not np.array_equal(toks, plain)
    assert np.all(toks[2::3] == FORCED) and np.all(toks[0::3] % 3 == 0) and np.all(toks[1::3] % 3 == 1)
    twin, _ = prefilled(gm, prompt)
    inputs = [first] + toks[:-1].tolist()
    state = 0
    for s in range(40):
        y = auto.mask(gm.forward(twin, [inputs[s]], NP + s), state)
        assert toks[s] == gr.argmax_last(y), s
        state = auto.walk(state, toks[s])
    assert a.guide_state() == state == auto.walk_all(0, toks) == 40 % 3


def test_chunking_and_calls(fa, env):
    gm, cfg, prompt = env
    first, plain, auto, g = setup(fa, gm, cfg, prompt)
    a, _ = guided(gm, prompt, g)
    one = gm.decode_greedy(a, first, NP, 20)
    b, _ = guided(gm, prompt, g)
    t0 = gm.decode_greedy(b, first, NP, 10)
    assert b.guide_state() == auto.walk_all(0, t0)
    t1 = gm.decode_greedy(b, t0[-1], NP + 10, 10)
    assert np.array_equal(np.concatenate([t0, t1]), one) and b.guide_state() == a.guide_state() == auto.walk_all(0, one)
    # a run that stops at an EOS: the same prefix, the cache length an unguided EOS run leaves (the EOS forward counts), and the
    # state behind the EOS's own edge -- what ran after it is discarded
    eos = int(one[9])
    n = int(np.flatnonzero(one == eos)[0])
    c, _ = guided(gm, prompt, g)
    got = gm.decode_greedy(c, first, NP, 20, eos=eos)
    assert np.array_equal(got, one[:n]) and len(c) == NP + n + 1
    assert c.guide_state() == auto.walk_all(0, one[: n + 1])
    eos_p = int(plain[9])
    n_p = int(np.flatnonzero(plain == eos_p)[0])
    d, _ = prefilled(gm, prompt)
    assert np.array_equal(gm.decode_greedy(d, first, NP, 20, eos=eos_p), plain[:n_p]) and len(d) == NP + n_p + 1
    # a rollback: truncate leaves guide and state alone; with the state set again the run repeats
    s_end = a.guide_state()
    a.truncate(NP)
    assert a.guide_state() == s_end
    a.set_guide(g, 0)
    assert np.array_equal(gm.decode_greedy(a, first, NP, 20), one)
    # ... and from the middle: the state after 10 tokens
    a.truncate(NP + 10)
    a.set_guide(g, auto.walk_all(0, one[:10]))
    assert np.array_equal(gm.decode_greedy(a, one[9], NP + 10, 10), one[10:])


def test_sampled_decode(fa, env):
    gm, cfg, prompt = env
    first, plain, auto, g = setup(fa, gm, cfg, prompt)
    a, _ = guided(gm, prompt, g)
    toks = gm.decode_sample(a, first, NP, 24, **SAMPLER)               # (draws_done = 1: the prefill's draw)
    assert len(toks) == 24
    twin, _ = prefilled(gm, prompt)
    inp, state = first, 0
    for s in range(24):
        y = auto.mask(gm.forward(twin, [inp], NP + s), state)
        want = fa.op_sample(y, 1, SAMPLER["temperature"], seed=SAMPLER["seed"], draws_done=1 + s, top_p=SAMPLER["top_p"])[0]
        assert toks[s] == want, s
        inp, state = int(toks[s]), auto.walk(state, toks[s])
    assert a.guide_state() == state
    # every step in state 2 returns the single allowed id whatever the seed
    for seed in (0, 11, 12345):
        b, _ = guided(gm, prompt, g)
        other = gm.decode_sample(b, first, NP, 12, temperature=1.5, seed=seed)
        assert np.all(other[2::3] == FORCED) and np.all(other[0::3] % 3 == 0) and np.all(other[1::3] % 3 == 1), seed


def test_rules_and_guide_together(fa, env):
    """Rules first, mask last.  The bias favours id 1 by +50: it wins wherever the guide allows it (state 1) and stays out where it
    does not (states 0 and 2)."""
    gm, cfg, prompt = env
    V = cfg["vocab_size"]
    first, plain, auto, g = setup(fa, gm, cfg, prompt)
    rules = dict(PEN, logit_bias={1: 50.0, 3: float("-inf")})
    a, _ = guided(gm, prompt, g)
    a.set_logit_rules(prompt_ids=prompt, **rules)
    toks = gm.decode_greedy(a, first, NP, 18)
    twin, _ = prefilled(gm, prompt)
    words, bias = lr.table(V, prompt_ids=prompt, logit_bias=rules["logit_bias"])
    inp, state = first, 0
    for s in range(18):
        lr.count(words, inp)
        y = auto.mask(lr.apply(gm.forward(twin, [inp], NP + s), words, bias, PEN["repetition_penalty"], PEN["frequency_penalty"], PEN["presence_penalty"]), state)
        assert toks[s] == gr.argmax_last(y), s
        inp, state = int(toks[s]), auto.walk(state, toks[s])
    assert a.guide_state() == state and np.array_equal(a.logit_counts(), words)
    assert toks[1] == 1 and 1 not in toks[0::3].tolist() + toks[2::3].tolist() and 3 not in toks.tolist()


def test_logprobs_stay_the_models_own(fa, env):
    gm, cfg, prompt = env
    first, plain, auto, g = setup(fa, gm, cfg, prompt)
    want = gm.decode_greedy(guided(gm, prompt, g)[0], first, NP, 12)
    a, _ = guided(gm, prompt, g)
    toks, tl, ids, lps = gm.decode_sample(a, first, NP, 12, 0.0, logprobs=5)
    assert np.array_equal(toks, want) and a.guide_state() == 0
    twin, _ = prefilled(gm, prompt)
    for s, t in enumerate(toks):
        row = gm.forward(twin, [first if s == 0 else toks[s - 1]], NP + s)
        lc.check_row(row, t, 5, tl[s], ids[s], lps[s], what=("guide + logprobs", s))
    # ... and the prefill form: the guided token, the raw row's values
    b, twin2 = gm.new_cache(CAP), gm.new_cache(CAP)
    b.set_guide(g, 2)
    tok, tl, ids, lps = gm.forward_sample(b, prompt, 0, 0.0, logprobs=5)
    assert tok == FORCED
    lc.check_row(gm.forward(twin2, prompt, 0), tok, 5, tl[0], ids[0], lps[0], what="prefill")


def test_nothing_changes_without_a_guide(fa, env):
    """The kernel list of a plain decode before an install and after install + removal is the same list, and the guide launch (form
    (a): mask and advance in one) appears exactly once per step only while a guide is installed."""
    gm, cfg, prompt = env
    first, plain, auto, g = setup(fa, gm, cfg, prompt)
    c, _ = prefilled(gm, prompt)
    count = lambda stats, name: sum(s["launches"] for s in stats if s["name"] == name)
    names = lambda stats: sorted((s["name"], s["launches"]) for s in stats)
    gm.profile_begin(); t0 = gm.decode_greedy(c, first, NP, 4); before = gm.profile_end()
    c.truncate(NP)
    c.set_guide(g, 0)
    gm.profile_begin(); t1 = gm.decode_greedy(c, first, NP, 4); with_guide = gm.profile_end()
    c.truncate(NP)                                                      # (leaves the guide alone)
    c.set_guide(g, 0)
    gm.profile_begin(); t2 = gm.decode_greedy(c, first, NP, 4); again = gm.profile_end()
    c.truncate(NP)
    c.clear_guide()
    gm.profile_begin(); t3 = gm.decode_greedy(c, first, NP, 4); after = gm.profile_end()
    assert names(before) == names(after) and np.array_equal(t0, t3) and np.array_equal(t0, plain[:4])
    assert count(before, "select_advance[guide]") == 0 and count(after, "select_advance[guide]") == 0
    for stats in (with_guide, again):
        assert count(stats, "select_advance[guide]") == 4 and count(stats, "select_advance") == 4
        assert count(stats, "select_advance[guide_ctl]") == 1           # one chunk: the host's state written once
        rest = [x for x in names(stats) if x[0] not in ("select_advance[guide]", "select_advance[guide_ctl]")]
        assert rest == names(before)
    assert t1[0] != t0[0] and np.array_equal(t1, t2)
    # the graph-replayed plain decode after a removal is the plain decode too
    c.truncate(NP)
    assert np.array_equal(gm.decode_greedy(c, first, NP, 40), plain)
    with pytest.raises(fa.FastLLMError):
        c.guide_state()                                                 # no guide installed


@pytest.mark.parametrize("B", [2, 4])
def test_batch(fa, env, B):
    """Odd members are guided (each from another start state), even ones are not; B = 2 and B = 4 are the two forms of the batch
    step.  Three batches over caches with the same history: `bg` with the guides, `bp` without any, `bt` the twin whose forward gives
    the raw rows."""
    gm, cfg, prompt = env
    lens = [NP, 5, 7, 6][:B]

    def fresh(n):
        c = gm.new_cache(CAP)
        return c, gm.forward_argmax(c, prompt[:n], 0)

    sets = [[fresh(n) for n in lens] for _ in range(3)]                 # guided, plain, twin
    firsts = [f for _, f in sets[0]]
    bg, bp, bt = (fa.Batch(gm, [c for c, _ in s]) for s in sets)
    plain = bp.decode_each(firsts, lens, 12)
    auto = automaton(cfg["vocab_size"], plain[1][0])
    g = fa.Guide(gm, *auto.csr())
    start = {i: (i // 2) % 3 for i in range(1, B, 2)}                   # member 1 starts in state 0, member 3 in state 1

    def check(got, plain, firsts, pos, states, what):
        """states: {member: state before the call}; returns them after it"""
        for i in range(B):
            assert len(got[i]) == 12
            if i not in states:
                assert np.array_equal(got[i], plain[i]), (what, i)      # an unguided member: the batch without any guide
        states = dict(states)
        for s in range(12):
            inp = [firsts[i] if s == 0 else int(got[i][s - 1]) for i in range(B)]
            lg, _ = bt.forward(inp, [p + s for p in pos])
            for i in range(B):
                y = auto.mask(lg[i], states[i]) if i in states else lg[i]
                assert got[i][s] == gr.argmax_last(y), (what, i, s)
                if i in states:
                    states[i] = auto.walk(states[i], got[i][s])
        return states

    for i, s in start.items():
        sets[0][i][0].set_guide(g, s)
    got = bg.decode_each(firsts, lens, 12)
    after = check(got, plain, firsts, lens, start, "batch")
    assert got[1][0] != plain[1][0]
    for i in start:
        assert sets[0][i][0].guide_state() == after[i], i
        # ... and the member's single-stream guided run
        c, f = fresh(lens[i])
        c.set_guide(g, start[i])
        assert f == firsts[i] and np.array_equal(gm.decode_greedy(c, f, lens[i], 12), got[i]) and c.guide_state() == after[i], i
    # replaced slots between two calls: an unguided cache takes guided member 1's place, a guided one unguided member 0's
    news = [[fresh(6), fresh(4)] for _ in range(3)]
    for bat, ((c0, _), (c1, _)) in zip((bg, bp, bt), news):
        bat.replace(1, c0)
        bat.replace(0, c1)
    news[0][1][0].set_guide(g, 2)
    pos2 = [lens[i] + 12 for i in range(B)]
    pos2[1], pos2[0] = 6, 4
    firsts2 = [int(got[i][-1]) for i in range(B)]
    firsts2[1], firsts2[0] = news[0][0][1], news[0][1][1]
    for k in (1, 2):                                                    # the other two batches follow the guided one's history
        for i in range(2, B):
            sets[k][i][0].copy_prefix(sets[0][i][0], len(sets[0][i][0]))
    states2 = {i: after[i] for i in start if i != 1}
    states2[0] = 2
    plain2 = bp.decode_each(firsts2, pos2, 12)
    got2 = bg.decode_each(firsts2, pos2, 12)
    after2 = check(got2, plain2, firsts2, pos2, states2, "after replace")
    assert got2[0][0] == FORCED and news[0][1][0].guide_state() == after2[0]
    for bat in (bg, bp, bt):
        bat.close()


def test_refusals(fa, env):
    gm, cfg, prompt = env
    V = cfg["vocab_size"]
    first, plain, auto, g = setup(fa, gm, cfg, prompt)
    c, _ = guided(gm, prompt, g, 1)
    other, _ = prefilled(gm, prompt)

    def refused(code, fn):
        with pytest.raises(fa.FastLLMError) as e:
            fn()
        assert e.value.code == code, str(e.value)

    refused(-10, lambda: gm.forward_verify(c, first, [1, 2], NP))
    refused(-10, lambda: gm.forward_verify(c, first, [], NP))
    refused(-10, lambda: gm.decode_lookup(c, prompt, first, NP, 4))
    assert len(c) == NP and c.guide_state() == 1
    e1, e2 = gm.new_cache(CAP), gm.new_cache(CAP)
    e2.set_guide(g, 0)
    refused(-10, lambda: gm.prefill_packed([e1, e2], [prompt, prompt[:5]]))
    assert len(e1) == 0 and len(e2) == 0 and e2.guide_state() == 0
    bat = fa.Batch(gm, [other, c])
    refused(-10, lambda: bat.forward([first, first], [NP, NP]))
    assert len(c) == NP and len(other) == NP and c.guide_state() == 1
    bat.close()
    # argument errors: a state the guide does not have, an id the model does not have; the cache stays as it was
    refused(-8, lambda: c.set_guide(g, 3))
    refused(-8, lambda: fa.Guide(gm, [0, 1], [V], [0]))
    refused(-8, lambda: fa.Guide(gm, [0, 2], [4, 4], [0, 0]))
    assert c.guide_state() == 1
    # the creator's reference goes; the caches that have the guide installed keep working
    want = gm.decode_greedy(guided(gm, prompt, g, 1)[0], first, NP, 9)
    g.close()
    assert np.array_equal(gm.decode_greedy(c, first, NP, 9), want) and c.guide_state() == (1 + 9) % 3
    c.clear_guide()
    c.truncate(NP)
    assert np.array_equal(gm.decode_greedy(c, first, NP, 9), plain[:9])


def test_tensor_parallel_is_refused(fa):
    cfg = synth.CONFIGS["llama_a"]
    gm = fa.Model(cfg, synth.synth_weights(cfg), dtype="bf16", tp_mode=fa.binding.TP_EMULATED, tp_size=2)
    auto = automaton(cfg["vocab_size"], 0)
    with pytest.raises(fa.FastLLMError) as e:
        fa.Guide(gm, *auto.csr())
    assert e.value.code == -10
    with pytest.raises(fa.FastLLMError) as e:                          # an argument error stays an argument error
        fa.Guide(gm, [0, 0], [], [])
    assert e.value.code == -8
    # a guide of another (single-GPU) model cannot be installed either, and the cache is left as it was
    one = fa.Model(cfg, synth.synth_weights(cfg), dtype="bf16")
    g = fa.Guide(one, *auto.csr())
    c = gm.new_cache(CAP)
    with pytest.raises(fa.FastLLMError):
        c.set_guide(g, 0)
    prompt = synth.prompt_ids(cfg, NP)
    assert gm.forward_argmax(c, prompt, 0) < cfg["vocab_size"] and len(c) == NP


# ---- the C++ host mirror (fastllm_host.hpp): generate_ids / generate_stream_ids with GuideOptions, a StreamBatcher request with one
GUIDE_ARGS = [C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32]


def guide_args(auto, start=0):
    rp, tk, nx = auto.csr()
    return (rp, tk, nx), [auto.n_states, rp.ctypes.data, tk.ctypes.data, nx.ctypes.data, start]


def generate_guided(host, h, prompt, n, auto, temperature=0.0, stream=0):  # noqa: F811
    host.flh_generate_guide.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_float, C.c_int64, C.c_double, C.c_int64] + GUIDE_ARGS + \
                                       [C.c_int, C.c_void_p, C.POINTER(C.c_size_t)]
    p = np.ascontiguousarray(prompt, dtype=np.uint32)
    out = np.zeros(n, np.uint32)
    n_out = C.c_size_t(0)
    keep, args = guide_args(auto)
    rc = host.flh_generate_guide(h, p.ctypes.data, p.size, n, temperature, -1, 0.0, 0, *args, stream, out.ctypes.data, C.byref(n_out))
    assert rc == 0, host.flh_last_error()
    return out[: n_out.value]


@pytest.mark.parametrize("temperature", [0.0, 0.8])
def test_host_mirror_generate_ids_with_a_guide(fa, host, monkeypatch, temperature):  # noqa: F811
    from test_gpu_host_mirror import generate, make
    monkeypatch.setenv("FASTLLM_POS_MODE", "tokens")
    monkeypatch.setenv("FASTLLM_MAX_SEQ", "64")
    h, cfg, w = make(host, "llama_a", dtype=0)
    prompt = synth.prompt_ids(cfg, NP)
    plain, _ = generate(host, h, prompt, 10, temperature=temperature)
    auto = automaton(cfg["vocab_size"], plain[0])
    got = generate_guided(host, h, prompt, 10, auto, temperature)
    gm = fa.Model(cfg, w, dtype="f32")
    c = gm.new_cache(64)
    c.set_guide(fa.Guide(gm, *auto.csr()), 0)
    t0 = gm.forward_sample(c, prompt, 0, temperature)
    t1 = gm.decode_sample(c, t0, NP, 9, temperature, seed=0, draws_done=1)
    assert len(got) == 10 and np.array_equal(got, np.concatenate([[t0], t1])) and got[0] != plain[0]
    assert np.all(got[2::3] == FORCED)
    assert np.array_equal(generate_guided(host, h, prompt, 10, auto, temperature, stream=1), got)
    host.flh_model_destroy(h)


def test_stream_batcher_with_a_guided_request(host, monkeypatch):  # noqa: F811
    """Two requests through two slots, one of them guided: each gets the tokens of its own single-stream run.  fp32 only: a slot's
    row in the batch step and the single stream's row agree to ~1e-6 there, while in bf16 the two steps may separate on a near-tie,
    which would say nothing about the guide."""
    from test_gpu_host_mirror import BATCH_DONE_CB, BATCH_TOKEN_CB, generate, make
    monkeypatch.setenv("FASTLLM_POS_MODE", "tokens")
    monkeypatch.setenv("FASTLLM_MAX_SEQ", "96")
    h, cfg, w = make(host, "llama_a", dtype=0)
    prompts = [synth.prompt_ids(cfg, n, seed=60 + i) for i, n in enumerate((9, 5))]
    ns = [14, 10]
    plain = [generate(host, h, p, n)[0] for p, n in zip(prompts, ns)]
    auto = automaton(cfg["vocab_size"], plain[1][0])
    alone = [plain[0], generate_guided(host, h, prompts[1], ns[1], auto)]
    assert alone[1][0] != plain[1][0]
    host.flh_batcher_create.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.POINTER(C.c_void_p)]
    host.flh_batcher_submit_guide.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_float, C.c_int64] + GUIDE_ARGS + \
                                             [BATCH_TOKEN_CB, BATCH_DONE_CB, C.c_void_p, C.POINTER(C.c_uint64)]
    host.flh_batcher_submit.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_float, C.c_int64, BATCH_TOKEN_CB, BATCH_DONE_CB, C.c_void_p,
                                        C.POINTER(C.c_uint64)]
    host.flh_batcher_run.argtypes = [C.c_void_p, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
    host.flh_batcher_destroy.argtypes = [C.c_void_p]
    b = C.c_void_p()
    assert host.flh_batcher_create(h, 2, 96, 4, C.byref(b)) == 0, host.flh_last_error()
    got, done = {}, {}

    def on_token(rid, tok, _user):
        got[rid].append(int(tok))
        return 1

    def on_done(rid, n, _user):
        done[rid] = int(n)
    cb, dcb = BATCH_TOKEN_CB(on_token), BATCH_DONE_CB(on_done)
    rids = []
    keep, args = guide_args(auto)
    for i in range(2):
        p = np.ascontiguousarray(prompts[i], dtype=np.uint32)
        rid = C.c_uint64(0)
        if i == 0:
            rc = host.flh_batcher_submit(b, p.ctypes.data, p.size, ns[i], 0.0, -1, cb, dcb, None, C.byref(rid))
        else:
            rc = host.flh_batcher_submit_guide(b, h, p.ctypes.data, p.size, ns[i], 0.0, -1, *args, cb, dcb, None, C.byref(rid))
        assert rc == 0, host.flh_last_error()
        got[rid.value] = []
        rids.append(rid.value)
    steps, pre = C.c_size_t(0), C.c_size_t(0)
    assert host.flh_batcher_run(b, C.byref(steps), C.byref(pre)) == 0, host.flh_last_error()
    host.flh_batcher_destroy(b)
    for i, rid in enumerate(rids):
        np.testing.assert_array_equal(np.asarray(got[rid], np.uint32), alone[i], err_msg="request %d" % i)
        assert done[rid] == len(alone[i])
    assert pre.value == 2
    host.flh_model_destroy(h)
