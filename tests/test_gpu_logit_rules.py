"""Logit rules through the model (fl_cache_set_logit_rules: logit_bias and repetition / frequency / presence penalties applied on the
device, the output counts kept by the decode step itself), bf16 and fp32.

Yardstick for a step: the numpy float32 restatement of tests/logit_rules_ref.py applied to the row fl_forward (or fl_batch_forward)
returns for the same step on a TWIN cache without rules fed the same ids -- the forward is deterministic, so that row holds the bits
the kernel read -- with the table (prompt bits, output counts) maintained by the test.  All comparisons are exact."""
import ctypes as C

import numpy as np
import pytest

import logit_rules_ref as lr
import logprob_cases as lc
import synth
from test_host_mirror import host  # noqa: F401

pytestmark = pytest.mark.gpu
CAP = 96
NP = 8                                       # prompt length
NEG = float("-inf")
PEN = dict(repetition_penalty=1.3, frequency_penalty=0.5, presence_penalty=0.25)
SAMPLER = dict(temperature=0.8, top_p=0.9, seed=3)


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


def prefilled(gm, prompt):
    c = gm.new_cache(CAP)
    return c, gm.forward_argmax(c, prompt, 0)


def pen(rules):
    return rules["repetition_penalty"], rules["frequency_penalty"], rules["presence_penalty"]


def two_biases(banned):
    """Two bias entries: `banned` can no longer be produced, and another id is favoured."""
    return {int(banned): NEG, (5 if int(banned) != 5 else 6): 1.5}


class Teacher:
    """The test's own table of one ruled stream, and the adjusted row of each of its steps."""

    def __init__(self, V, prompt, rules):
        self.words, self.bias = lr.table(V, prompt_ids=prompt, logit_bias=rules.get("logit_bias"))
        self.pen = pen(rules)

    def step(self, raw_row, input_token):
        lr.count(self.words, input_token)
        return lr.apply(raw_row, self.words, self.bias, *self.pen)


def ruled(gm, prompt, rules):
    """A cache prefilled WITHOUT rules (so every stream of a test starts from the same first token), then given them."""
    c, first = prefilled(gm, prompt)
    c.set_logit_rules(prompt_ids=prompt, **rules)
    return c, first


def setup(gm, prompt):
    """The unruled greedy run, and rules that make the ruled run differ from it at its first step."""
    c, first = prefilled(gm, prompt)
    plain = gm.decode_greedy(c, first, NP, 40)
    return first, plain, dict(PEN, logit_bias=two_biases(plain[0]))


def test_prefill(env):
    gm, cfg, prompt = env
    V = cfg["vocab_size"]
    a, b, c, twin = (gm.new_cache(CAP) for _ in range(4))
    plain = gm.forward_sample(a, prompt, 0, 0.0)
    for cache in (b, c):
        cache.set_logit_rules(logit_bias={plain: NEG})
    row = gm.forward(twin, prompt, 0)
    words, bias = lr.table(V, logit_bias={plain: NEG})
    want = lr.argmax_last(lr.apply(row, words, bias))
    got = gm.forward_sample(b, prompt, 0, 0.0)
    assert got != plain and got == want and gm.forward_argmax(c, prompt, 0) == want
    assert len(b) == len(c) == NP and not b.logit_counts().any()       # a forward counts nothing
    # fl_forward on a ruled cache returns the model's own row
    assert np.array_equal(lr.bits(gm.forward(b, [got], NP)), lr.bits(gm.forward(twin, [got], NP)))


def test_greedy_decode_40_steps_in_two_chunks(env):
    gm, cfg, prompt = env
    V = cfg["vocab_size"]
    first, plain, rules = setup(gm, prompt)
    free = gm.decode_greedy(ruled(gm, prompt, rules)[0], first, NP, 40)
    eos = next(i for i in range(V) if i not in set(free.tolist()) and i != first)      # an id that never occurs: chunks of 16 + 24
    a, _ = ruled(gm, prompt, rules)
    toks = gm.decode_greedy(a, first, NP, 40, eos=eos)
    assert len(toks) == 40 and np.array_equal(toks, free) and len(a) == NP + 40
    assert not np.array_equal(toks, plain)
    twin, _ = prefilled(gm, prompt)
    t = Teacher(V, prompt, rules)
    inputs = [first] + toks[:-1].tolist()
    for s in range(40):
        y = t.step(gm.forward(twin, [inputs[s]], NP + s), inputs[s])
        assert toks[s] == lr.argmax_last(y), s
    counts = np.bincount(inputs, minlength=V).astype(np.uint32)
    counts[np.unique(prompt)] |= lr.PROMPT_BIT
    got = a.logit_counts()
    assert np.array_equal(got, counts) and np.array_equal(got, t.words)


def test_sampled_decode(fa, env):
    gm, cfg, prompt = env
    first, plain, rules = setup(gm, prompt)
    a, _ = ruled(gm, prompt, rules)
    toks = gm.decode_sample(a, first, NP, 24, **SAMPLER)               # (draws_done = 1: the prefill's draw)
    assert len(toks) == 24
    twin, _ = prefilled(gm, prompt)
    t = Teacher(cfg["vocab_size"], prompt, rules)
    inp = first
    for s in range(24):
        y = t.step(gm.forward(twin, [inp], NP + s), inp)
        want = fa.op_sample(y, 1, SAMPLER["temperature"], seed=SAMPLER["seed"], draws_done=1 + s, top_p=SAMPLER["top_p"])[0]
        assert toks[s] == want, s
        inp = int(toks[s])


def test_chunking_and_calls(env):
    gm, cfg, prompt = env
    first, plain, rules = setup(gm, prompt)
    one = gm.decode_greedy(ruled(gm, prompt, rules)[0], first, NP, 20)
    b, _ = ruled(gm, prompt, rules)
    t0 = gm.decode_greedy(b, first, NP, 10)
    t1 = gm.decode_greedy(b, t0[-1], NP + 10, 10)
    assert np.array_equal(np.concatenate([t0, t1]), one)
    # a run that stops at an EOS: the same prefix, and the cache length an unruled EOS run leaves (the EOS forward counts)
    eos = int(one[9])
    n = int(np.flatnonzero(one == eos)[0])
    c, _ = ruled(gm, prompt, rules)
    got = gm.decode_greedy(c, first, NP, 20, eos=eos)
    assert np.array_equal(got, one[:n]) and len(c) == NP + n + 1
    eos_p = int(plain[9])
    n_p = int(np.flatnonzero(plain == eos_p)[0])
    d, _ = prefilled(gm, prompt)
    assert np.array_equal(gm.decode_greedy(d, first, NP, 20, eos=eos_p), plain[:n_p]) and len(d) == NP + n_p + 1


def test_logprobs_stay_the_models_own(env):
    gm, cfg, prompt = env
    first, plain, rules = setup(gm, prompt)
    want = gm.decode_greedy(ruled(gm, prompt, rules)[0], first, NP, 12)
    a, _ = ruled(gm, prompt, rules)
    toks, tl, ids, lps = gm.decode_sample(a, first, NP, 12, 0.0, logprobs=5)
    assert np.array_equal(toks, want)
    twin, _ = prefilled(gm, prompt)
    for s, t in enumerate(toks):
        row = gm.forward(twin, [first if s == 0 else toks[s - 1]], NP + s)
        lc.check_row(row, t, 5, tl[s], ids[s], lps[s], what=("rules + logprobs", s))
    # ... and the prefill form: the ruled token, the raw row's values
    b, twin2 = gm.new_cache(CAP), gm.new_cache(CAP)
    b.set_logit_rules(logit_bias={first: NEG})
    tok, tl, ids, lps = gm.forward_sample(b, prompt, 0, 0.0, logprobs=5)
    assert tok != first
    lc.check_row(gm.forward(twin2, prompt, 0), tok, 5, tl[0], ids[0], lps[0], what="prefill")


def test_nothing_changes_without_rules(env):
    """The kernel list of a plain decode before an install and after install + removal is the same list, and the rules launch
    appears exactly once per step only while rules are installed."""
    gm, cfg, prompt = env
    first, plain, rules = setup(gm, prompt)
    c, _ = prefilled(gm, prompt)
    count = lambda stats, name: sum(s["launches"] for s in stats if s["name"] == name)
    names = lambda stats: sorted((s["name"], s["launches"]) for s in stats)
    gm.profile_begin(); t0 = gm.decode_greedy(c, first, NP, 4); before = gm.profile_end()
    c.truncate(NP)
    c.set_logit_rules(prompt_ids=prompt, **rules)
    gm.profile_begin(); t1 = gm.decode_greedy(c, first, NP, 4); with_rules = gm.profile_end()
    c.truncate(NP)                                                      # (leaves the rules alone)
    gm.profile_begin(); t2 = gm.decode_greedy(c, first, NP, 4); again = gm.profile_end()
    c.truncate(NP)
    c.clear_logit_rules()
    gm.profile_begin(); t3 = gm.decode_greedy(c, first, NP, 4); after = gm.profile_end()
    assert names(before) == names(after) and np.array_equal(t0, t3) and np.array_equal(t0, plain[:4])
    assert count(before, "select_advance[rules]") == 0 and count(after, "select_advance[rules]") == 0
    for stats in (with_rules, again):
        assert count(stats, "select_advance[rules]") == 4 and count(stats, "select_advance") == 4
        rest = [x for x in names(stats) if x[0] not in ("select_advance[rules]", "select_advance[rules_ctl]")]
        assert rest == names(before)
    assert t1[0] != t0[0] and t2[0] != t0[0]                            # (the rules ban the plain run's first token)
    # the graph-replayed plain decode after a removal is the plain decode too
    c.truncate(NP)
    assert np.array_equal(gm.decode_greedy(c, first, NP, 40), plain)


@pytest.mark.parametrize("B", [2, 4])
def test_batch(fa, env, B):
    """Member 0 has no rules, the others each their own; B = 2 and B = 4 are the two forms of the batch step.  Three batches over
    caches with the same history: `br` with the rules, `bp` without any, `bt` the twin whose forward gives the raw rows."""
    gm, cfg, prompt = env
    V = cfg["vocab_size"]
    lens = [NP, 5, 7, 6][:B]

    def member_rules(i, banned):
        return dict(repetition_penalty=1.1 + 0.1 * i, frequency_penalty=0.2 * i, presence_penalty=0.1 * i, logit_bias=two_biases(banned))

    def fresh(n):
        c = gm.new_cache(CAP)
        return c, gm.forward_argmax(c, prompt[:n], 0)

    sets = [[fresh(n) for n in lens] for _ in range(3)]                 # ruled, plain, twin
    firsts = [f for _, f in sets[0]]
    br, bp, bt = (fa.Batch(gm, [c for c, _ in s]) for s in sets)
    teachers = [None] * B

    def check(got, plain, firsts, pos, differ, what):
        assert np.array_equal(got[0], plain[0]) and all(len(g) == 12 for g in got), what
        for i in differ:
            assert got[i][0] != plain[i][0], (what, i)                  # (its rules ban the plain run's first token)
        for s in range(12):
            inp = [firsts[i] if s == 0 else int(got[i][s - 1]) for i in range(B)]
            lg, _ = bt.forward(inp, [p + s for p in pos])
            for i in range(B):
                y = lg[i] if teachers[i] is None else teachers[i].step(lg[i], inp[i])
                assert got[i][s] == lr.argmax_last(y), (what, i, s)

    plain = bp.decode_each(firsts, lens, 12)
    for i in range(1, B):
        rules = member_rules(i, plain[i][0])
        sets[0][i][0].set_logit_rules(prompt_ids=prompt[: lens[i]], **rules)
        teachers[i] = Teacher(V, prompt[: lens[i]], rules)
    got = br.decode_each(firsts, lens, 12)
    check(got, plain, firsts, lens, range(1, B), "batch")
    for i in range(1, B):
        assert np.array_equal(sets[0][i][0].logit_counts(), teachers[i].words), i
    # a replaced slot: a ruled cache joins the ruled batch (an unruled one the other two); the other members' counts carry on
    slot = B - 1
    news = [fresh(6) for _ in range(3)]
    for bat, (c, _) in zip((br, bp, bt), news):
        bat.replace(slot, c)
    pos2 = [lens[i] + 12 for i in range(B)]
    pos2[slot] = 6
    firsts2 = [int(got[i][-1]) for i in range(B)]
    firsts2[slot] = news[0][1]
    plain2 = bp.decode_each(firsts2, pos2, 12)
    new_rules = dict(repetition_penalty=0.7, frequency_penalty=-0.3, presence_penalty=0.4, logit_bias=two_biases(plain2[slot][0]))
    news[0][0].set_logit_rules(prompt_ids=prompt[:6], **new_rules)
    teachers[slot] = Teacher(V, prompt[:6], new_rules)
    got2 = br.decode_each(firsts2, pos2, 12)
    check(got2, plain2, firsts2, pos2, [slot], "after replace")
    assert np.array_equal(news[0][0].logit_counts(), teachers[slot].words)


def test_refusals(fa, env):
    gm, cfg, prompt = env
    V = cfg["vocab_size"]
    c, first = ruled(gm, prompt, dict(PEN))
    other, _ = prefilled(gm, prompt)

    def refused(code, fn):
        with pytest.raises(fa.FastLLMError) as e:
            fn()
        assert e.value.code == code, str(e.value)

    refused(-10, lambda: gm.forward_verify(c, first, [1, 2], NP))
    refused(-10, lambda: gm.forward_verify(c, first, [], NP))
    refused(-10, lambda: gm.decode_lookup(c, prompt, first, NP, 4))
    assert len(c) == NP
    e1, e2 = gm.new_cache(CAP), gm.new_cache(CAP)
    e2.set_logit_rules(logit_bias={3: 1.0})
    refused(-10, lambda: gm.prefill_packed([e1, e2], [prompt, prompt[:5]]))
    assert len(e1) == 0 and len(e2) == 0
    bat = fa.Batch(gm, [other, c])
    refused(-10, lambda: bat.forward([first, first], [NP, NP]))
    assert len(c) == NP and len(other) == NP
    # argument errors leave the cache as it was: its rules and its table
    before = c.logit_counts()
    refused(-8, lambda: c.set_logit_rules(logit_bias={V: 1.0}))
    refused(-8, lambda: c.set_logit_rules(prompt_ids=[0, V]))
    refused(-8, lambda: c.set_logit_rules(output_ids=[V + 7]))
    refused(-8, lambda: c.set_logit_rules(logit_bias=[(4, 1.0), (4, 2.0)]))
    refused(-8, lambda: c.set_logit_rules(repetition_penalty=0.0))
    assert np.array_equal(c.logit_counts(), before)
    refused(-8, lambda: other.logit_counts())                           # no rules installed
    # output_ids seed the counts
    other.set_logit_rules(prompt_ids=[1, 2], output_ids=[2, 2, 9])
    w = other.logit_counts()
    assert w[1] == lr.PROMPT_BIT and w[2] == (lr.PROMPT_BIT | 2) and w[9] == 1 and w.sum(dtype=np.uint64) == int(lr.PROMPT_BIT) * 2 + 3
    bat.close()


def test_tensor_parallel_is_refused(fa):
    cfg = synth.CONFIGS["llama_a"]
    gm = fa.Model(cfg, synth.synth_weights(cfg), dtype="bf16", tp_mode=fa.binding.TP_EMULATED, tp_size=2)
    c = gm.new_cache(CAP)
    with pytest.raises(fa.FastLLMError) as e:
        c.set_logit_rules(logit_bias={3: 1.0})
    assert e.value.code == -10 and len(c) == 0
    with pytest.raises(fa.FastLLMError) as e:                          # an argument error stays an argument error
        c.set_logit_rules(logit_bias={3: float("nan")})
    assert e.value.code == -8
    prompt = synth.prompt_ids(cfg, NP)
    assert gm.forward_argmax(c, prompt, 0) < cfg["vocab_size"] and len(c) == NP


# ---- the C++ host mirror (fastllm_host.hpp): generate_ids with LogitRules, StreamBatcher requests with LogitRules
RULE_ARGS = [C.c_size_t, C.c_void_p, C.c_void_p, C.c_float, C.c_float, C.c_float]


def rule_args(rules):
    ids = np.ascontiguousarray(list(rules["logit_bias"].keys()), dtype=np.uint32)
    vals = np.ascontiguousarray(list(rules["logit_bias"].values()), dtype=np.float32)
    return (ids, vals), [ids.size, ids.ctypes.data, vals.ctypes.data, rules["repetition_penalty"], rules["frequency_penalty"], rules["presence_penalty"]]


def generate_rules(host, h, prompt, n, rules, temperature=0.0):  # noqa: F811
    host.flh_generate_rules.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_float, C.c_int64, C.c_double, C.c_int64] + RULE_ARGS + \
                                       [C.c_void_p, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
    p = np.ascontiguousarray(prompt, dtype=np.uint32)
    out = np.zeros(n, np.uint32)
    n_out, fw = C.c_size_t(0), C.c_size_t(0)
    keep, args = rule_args(rules)
    rc = host.flh_generate_rules(h, p.ctypes.data, p.size, n, temperature, -1, 0.0, 0, *args, out.ctypes.data, C.byref(n_out), C.byref(fw))
    assert rc == 0, host.flh_last_error()
    assert fw.value == n_out.value
    return out[: n_out.value]


@pytest.mark.parametrize("temperature", [0.0, 0.8])
def test_host_mirror_generate_ids_with_rules(fa, host, monkeypatch, temperature):  # noqa: F811
    from test_gpu_host_mirror import generate, make
    monkeypatch.setenv("FASTLLM_POS_MODE", "tokens")
    monkeypatch.setenv("FASTLLM_MAX_SEQ", "64")
    h, cfg, w = make(host, "llama_a", dtype=0)
    prompt = synth.prompt_ids(cfg, NP)
    plain, _ = generate(host, h, prompt, 10, temperature=temperature)
    rules = dict(PEN, logit_bias=two_biases(plain[1]))
    got = generate_rules(host, h, prompt, 10, rules, temperature)
    gm = fa.Model(cfg, w, dtype="f32")
    c = gm.new_cache(64)
    c.set_logit_rules(prompt_ids=prompt, **rules)
    t0 = gm.forward_sample(c, prompt, 0, temperature)
    t1 = gm.decode_sample(c, t0, NP, 9, temperature, seed=0, draws_done=1)
    assert len(got) == 10 and np.array_equal(got, np.concatenate([[t0], t1])) and not np.array_equal(got, plain)
    host.flh_model_destroy(h)


def test_stream_batcher_with_ruled_requests(host, monkeypatch):  # noqa: F811
    """Four requests through two slots, two of them with logit rules: each gets the tokens of its own single-stream run.  fp32 only:
    a slot's row in the batch step and the single stream's row agree to ~1e-6 there, while in bf16 the two steps may separate on a
    near-tie, which would say nothing about the rules."""
    from test_gpu_host_mirror import BATCH_DONE_CB, BATCH_TOKEN_CB, generate, make
    monkeypatch.setenv("FASTLLM_POS_MODE", "tokens")
    monkeypatch.setenv("FASTLLM_MAX_SEQ", "96")
    h, cfg, w = make(host, "llama_a", dtype=0)
    prompts = [synth.prompt_ids(cfg, n, seed=60 + i) for i, n in enumerate((9, 5, 12, 7))]
    ns = [14, 10, 9, 16]
    plain = [generate(host, h, p, n)[0] for p, n in zip(prompts, ns)]
    rules = [None, dict(PEN, logit_bias=two_biases(plain[1][1])), None,
             dict(repetition_penalty=1.0, frequency_penalty=0.8, presence_penalty=-0.2, logit_bias=two_biases(plain[3][2]))]
    alone = [plain[i] if rules[i] is None else generate_rules(host, h, prompts[i], ns[i], rules[i]) for i in range(4)]
    assert not np.array_equal(alone[1], plain[1]) and not np.array_equal(alone[3], plain[3])
    host.flh_batcher_create.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.POINTER(C.c_void_p)]
    host.flh_batcher_submit_rules.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_float, C.c_int64] + RULE_ARGS + \
                                             [BATCH_TOKEN_CB, BATCH_DONE_CB, C.c_void_p, C.POINTER(C.c_uint64)]
    host.flh_batcher_submit.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_float, C.c_int64, BATCH_TOKEN_CB, BATCH_DONE_CB, C.c_void_p,
                                        C.POINTER(C.c_uint64)]
    host.flh_batcher_run.argtypes = [C.c_void_p, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
    host.flh_batcher_destroy.argtypes = [C.c_void_p]
    b = C.c_void_p()
    assert host.flh_batcher_create(h, 2, 96, 4, C.byref(b)) == 0, host.flh_last_error()
    got, done, keep = {}, {}, []

    def on_token(rid, tok, _user):
        got[rid].append(int(tok))
        return 1

    def on_done(rid, n, _user):
        done[rid] = int(n)
    cb, dcb = BATCH_TOKEN_CB(on_token), BATCH_DONE_CB(on_done)
    rids = []
    for i in range(4):
        p = np.ascontiguousarray(prompts[i], dtype=np.uint32)
        rid = C.c_uint64(0)
        if rules[i] is None:
            rc = host.flh_batcher_submit(b, p.ctypes.data, p.size, ns[i], 0.0, -1, cb, dcb, None, C.byref(rid))
        else:
            arrays, args = rule_args(rules[i])
            keep.append(arrays)
            rc = host.flh_batcher_submit_rules(b, p.ctypes.data, p.size, ns[i], 0.0, -1, *args, cb, dcb, None, C.byref(rid))
        assert rc == 0, host.flh_last_error()
        got[rid.value] = []
        rids.append(rid.value)
    steps, pre = C.c_size_t(0), C.c_size_t(0)
    assert host.flh_batcher_run(b, C.byref(steps), C.byref(pre)) == 0, host.flh_last_error()
    host.flh_batcher_destroy(b)
    for i, rid in enumerate(rids):
        np.testing.assert_array_equal(np.asarray(got[rid], np.uint32), alone[i], err_msg="request %d" % i)
        assert done[rid] == len(alone[i])
    assert pre.value == 4
    host.flh_model_destroy(h)
