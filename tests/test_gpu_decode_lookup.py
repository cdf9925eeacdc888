"""The speculative greedy loop (fl_decode_lookup) against fl_decode_greedy on a twin cache.

Acceptance is forced through the corpus: corpus = prompt ++ [first] ++ want makes almost every draft right; the same corpus with
every 5th id of the `want` part replaced makes regular rejections.

fp32: the loop returns exactly `want` -- no divergence is excused.  The prompt seeds were chosen on the CPU: at every one of the 48
steps the fp32 oracle's gap between its two largest logits exceeds 2e-3 x max(1, max|logit|), twice the project's 1e-3 fp32 bar (once
for each path); the test asserts that.  bf16: equal to `want`, or at the first difference k the gap of the top two logits (one-token
forwards of want[:k]) is below 4e-2 x max(1, max|logit|) -- the rule and the number of test_gpu_batch.py -- and at most ONE of the
parametrised bf16 cases may need that.

Greedy loops of random-weight models fall into cycles, and inside a cycle of period P the most recent earlier occurrence of the
n-gram lies P ids back, so a draft is at most P ids long whatever the corpus holds.  The seeds were therefore also chosen on the CPU
so that the rule itself (simulate() on the oracle's continuation, fp32 and bf16-rounded) meets the coverage the loop is asked for
with both n-gram settings: accepted / steps >= 3 and steps < 16 at max_draft 7 on the clean corpus, drafted > accepted > 0 on the
corrupted one.  test_seeds_keep_the_fp32_margin asserts that too.  Of seeds 100 - 399 those that pass were ranked by the bf16
oracle's smallest top-two gap over the 48 steps (0.4 % - 1.7 % of the logit range; no seed keeps 4 % for 48 steps), so whether a
bf16 case needs the excuse is not known from the CPU."""
import ctypes as C

import numpy as np
import pytest

import synth
from oracle import oracle
from test_gpu_host_mirror import FAM, generate, make  # noqa: F401
from test_host_mirror import config_json, host  # noqa: F401
from test_lookup_abi import lookup_draft_ref

pytestmark = pytest.mark.gpu

SEEDS = {"llama_a": 355, "mistral_a": 220, "qwen2_a": 357, "llama_mha": 368, "llama_d100": 219}
L, N, CAP = 12, 48, 96


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


def start(gm, name, cap=CAP):
    p = synth.prompt_ids(synth.CONFIGS[name], L, seed=SEEDS[name])
    c = gm.new_cache(cap)
    return c, p, gm.forward_argmax(c, p, 0)


def corpora(cfg, p, first, want):
    clean = np.concatenate([p, [first], want]).astype(np.uint32)
    bad = want.copy()
    bad[4::5] = (bad[4::5] + 1) % cfg["vocab_size"]
    return clean, np.concatenate([p, [first], bad]).astype(np.uint32)


def simulate(corpus, first, want, max_draft, ngram_max, ngram_min, window=None):
    """The loop's bookkeeping when every row's ArgMax is `want`'s: (steps, drafted, accepted) and the first index of every step."""
    hist = list(corpus) + [first]
    emitted, steps, drafted, accepted, starts = 0, 0, 0, 0, []
    while emitted < len(want):
        limit = len(want) - emitted - 1
        if window is not None:
            limit = min(limit, window)
        d = lookup_draft_ref(hist, max_draft, ngram_max, ngram_min, limit)
        n = 0
        while n < len(d) and d[n] == want[emitted + n]:
            n += 1
        starts.append(emitted)
        steps, drafted, accepted = steps + 1, drafted + len(d), accepted + n
        hist += [int(t) for t in want[emitted:emitted + n + 1]]
        emitted += n + 1
    return dict(steps=steps, drafted=drafted, accepted=accepted), starts


def same_or_near_tie(gm, name, got, want, case):
    """bf16: only a near-tie of the two largest logits may separate the two paths (test_gpu_batch.py's rule and number)."""
    assert len(got) == len(want)
    if np.array_equal(got, want):
        return
    k = int(np.argmax(got != want))
    c, p, first = start(gm, name)
    lg = None
    for s, t in enumerate([first] + want[:k].tolist()):
        lg = gm.forward(c, [t], L + s)
    top2 = np.sort(lg)[-2:]
    print("%s: differs from decode_greedy at %d, top-two gap %.3e of %.3e" % (case, k, top2[1] - top2[0], np.abs(lg).max()))
    assert top2[1] - top2[0] < 4e-2 * max(1.0, np.abs(lg).max()), "%s diverges at %d with a clear margin" % (case, k)
    _excused.add(case)
    assert len(_excused) <= 1, "more than one bf16 case needs the near-tie excuse: %s" % sorted(_excused)


def test_seeds_keep_the_fp32_margin():
    """CPU part of the fp32 claim: the oracle's top-two gap at each of the 48 steps (and at the prompt's own token), and that the
    drafting rule alone reaches the coverage asked of the loop on the oracle's continuation (no short cycle caps the drafts)."""
    for name, seed in SEEDS.items():
        cfg = synth.CONFIGS[name]
        om = oracle.OracleModel(cfg, synth.as_f32(synth.synth_weights(cfg)))
        toks, lg = om.generate(om.new_cache(CAP), synth.prompt_ids(cfg, L, seed=seed), N + 1, want_logits=True)
        s = np.sort(lg, axis=1)
        rel = (s[:, -1] - s[:, -2]) / np.maximum(1.0, np.abs(lg).max(axis=1))
        assert len(toks) == N + 1 and rel.min() > 2e-3, (name, rel.min())
        assert len(set(toks.tolist())) >= 8, name
        p, first, want = synth.prompt_ids(cfg, L, seed=seed), int(toks[0]), toks[1:]
        clean, bad = corpora(cfg, p, first, want)
        for ng in ((3, 1), (2, 2)):
            st, _ = simulate(clean, first, want, 7, ng[0], ng[1])
            assert st["accepted"] / st["steps"] >= 3 and st["steps"] < N / 3, (name, ng, st)
            st, _ = simulate(bad, first, want, 7, ng[0], ng[1])
            assert st["drafted"] > st["accepted"] > 0, (name, ng, st)


@pytest.mark.parametrize("name", list(SEEDS))
def test_lookup_loop_fp32_is_exactly_greedy(fa, name):
    cfg = synth.CONFIGS[name]
    gm = model(fa, name, "f32")
    twin, p, first = start(gm, name)
    want = gm.decode_greedy(twin, first, L, N)
    om = oracle.OracleModel(cfg, synth.as_f32(synth.synth_weights(cfg)))
    assert np.array_equal(np.concatenate([[first], want]), om.generate(om.new_cache(CAP), p, N + 1))     # the margin above holds on the GPU path
    clean, bad = corpora(cfg, p, first, want)
    for corpus, what in ((clean, "clean"), (bad, "corrupted")):
        for max_draft in (1, 7, 15):
            for ng in ((3, 1), (2, 2)):
                c, _, f = start(gm, name)
                got, st = gm.decode_lookup(c, corpus, f, L, N, max_draft=max_draft, ngram_max=ng[0], ngram_min=ng[1], return_stats=True)
                assert np.array_equal(got, want), (name, what, max_draft, ng)
                assert len(c) == L + N
                sim, _ = simulate(corpus, first, want, max_draft, ng[0], ng[1])
                assert st == sim, (name, what, max_draft, ng, st, sim)       # the drafts and the acceptance are the rule's
                if what == "clean" and max_draft == 7:
                    print("%s clean ngram %s: %s" % (name, ng, st))
                    assert st["accepted"] / st["steps"] >= 3 and st["steps"] < N / 3
                if what == "corrupted" and max_draft == 7:
                    assert st["drafted"] > st["accepted"] > 0
    c, _, f = start(gm, name)
    got, st = gm.decode_lookup(c, clean, f, L, N, max_draft=0, return_stats=True)
    assert np.array_equal(got, want) and st == dict(steps=N, drafted=0, accepted=0) and len(c) == L + N


@pytest.mark.parametrize("name", list(SEEDS))
def test_lookup_loop_bf16(fa, name):
    cfg = synth.CONFIGS[name]
    gm = model(fa, name, "bf16")
    twin, p, first = start(gm, name)
    want = gm.decode_greedy(twin, first, L, N)
    clean, bad = corpora(cfg, p, first, want)
    for corpus, what in ((clean, "clean"), (bad, "corrupted")):
        for max_draft in (1, 7, 15):
            for ng in ((3, 1), (2, 2)):
                c, _, f = start(gm, name)
                got, st = gm.decode_lookup(c, corpus, f, L, N, max_draft=max_draft, ngram_max=ng[0], ngram_min=ng[1], return_stats=True)
                assert len(c) == L + N
                same_or_near_tie(gm, name, got, want, "bf16 " + name)
                if np.array_equal(got, want) and max_draft == 7:
                    if what == "clean":
                        assert st["accepted"] / st["steps"] >= 3 and st["steps"] < N / 3
                    else:
                        assert st["drafted"] > st["accepted"] > 0
    c, _, f = start(gm, name)
    got, st = gm.decode_lookup(c, clean, f, L, N, max_draft=0, return_stats=True)
    assert np.array_equal(got, want) and st["steps"] == N           # plain greedy steps: the decode kernels, bit for bit


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("name", ["llama_a", "mistral_a", "qwen2_a"])
def test_eos_inside_an_accepted_run(fa, name, dtype):
    cfg = synth.CONFIGS[name]
    gm = model(fa, name, dtype)
    twin, p, first = start(gm, name)
    want = gm.decode_greedy(twin, first, L, N)
    clean, _ = corpora(cfg, p, first, want)
    _, starts = simulate(clean, first, want, 7, 3, 1)
    ends = starts[1:] + [N]
    # an index strictly inside a step (accepted drafts on both sides of it) whose token has not come up before
    i = next(i for s, e in zip(starts, ends) for i in range(s + 1, e - 1) if want[i] not in want[:i] and want[i] != first)
    c, _, f = start(gm, name)
    got = gm.decode_lookup(c, clean, f, L, N, eos=int(want[i]))
    if dtype == "f32":
        assert np.array_equal(got, want[:i])
    else:
        same_or_near_tie(gm, name, got, want[: len(got)], "bf16 eos " + name)
    assert len(c) == L + len(got) + (1 if len(got) < N else 0)         # the length fl_decode_greedy leaves
    if np.array_equal(got, want[:i]):
        t2, _, _ = start(gm, name)
        assert np.array_equal(gm.decode_greedy(t2, first, L, N, eos=int(want[i])), want[:i]) and len(t2) == len(c)
        if dtype == "f32":                                             # going on from there: the twin's tokens
            assert np.array_equal(gm.decode_greedy(c, int(want[i]), L + i + 1, 6), gm.decode_greedy(t2, int(want[i]), L + i + 1, 6))


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_room(fa, dtype):
    name = "mistral_a"
    cfg = synth.CONFIGS[name]
    gm = model(fa, name, dtype)
    twin, p, first = start(gm, name)
    want = gm.decode_greedy(twin, first, L, N)
    clean, _ = corpora(cfg, p, first, want)
    c, _, f = start(gm, name, cap=L + N)                               # exactly the room fl_decode_greedy needs
    got = gm.decode_lookup(c, clean, f, L, N, max_draft=15)
    assert len(got) == N and len(c) == L + N == c.capacity()
    if dtype == "f32":
        assert np.array_equal(got, want)
    c, _, f = start(gm, name, cap=L + N - 1)
    with pytest.raises(fa.FastLLMError) as e:
        gm.decode_lookup(c, clean, f, L, N)
    assert e.value.code == -7 and len(c) == L                          # FL_ERR_SEQ_OVERFLOW before anything ran


def test_fp8_model_matches_its_own_greedy_loop(fa):
    name = "mistral_a"
    cfg = synth.CONFIGS[name]
    gm = model(fa, name, "bf16", decode_weights="e4m3")
    twin, p, first = start(gm, name)
    want = gm.decode_greedy(twin, first, L, N)
    clean, _ = corpora(cfg, p, first, want)
    c, _, f = start(gm, name)
    got, st = gm.decode_lookup(c, clean, f, L, N, return_stats=True)
    assert len(c) == L + N and st["accepted"] > 0
    same_or_near_tie(gm, name, got, want, "bf16 e4m3 " + name)


@pytest.mark.parametrize("name", ["llama_a", "mistral_a", "qwen2_a"])
@pytest.mark.parametrize("mode", ["reference", "tokens"])
def test_host_mirror_lookup_overloads(host, name, mode, monkeypatch):
    """Model<M>::generate_ids / generate_stream_ids with LookupOptions (fp32): the ids of the plain greedy request; a temperature is refused."""
    monkeypatch.setenv("FASTLLM_POS_MODE", mode)
    monkeypatch.setenv("FASTLLM_MAX_SEQ", "96")
    host.flh_generate_lookup.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_float, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int,
                                         C.c_void_p, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t), C.c_void_p]
    h, cfg, _ = make(host, name, dtype=0)
    base = synth.prompt_ids(cfg, 10, seed=SEEDS[name])
    prompt = np.concatenate([base, base[1:], base[1:4]]).astype(np.uint32)       # a prompt that repeats itself: drafts from the prompt
    n = 24
    want, _ = generate(host, h, prompt, n)

    def lookup(stream, temperature=0.0, eos=-1):
        out = np.zeros(n, dtype=np.uint32)
        n_out, fw = C.c_size_t(0), C.c_size_t(0)
        st = (C.c_uint64 * 3)()
        rc = host.flh_generate_lookup(h, prompt.ctypes.data, prompt.size, n, temperature, eos, 7, 3, 1, stream, out.ctypes.data, C.byref(n_out),
                                      C.byref(fw), st)
        return rc, out[: n_out.value], fw.value, list(st)

    for stream in (0, 1):
        rc, got, fw, st = lookup(stream)
        assert rc == 0, host.flh_last_error()
        np.testing.assert_array_equal(got, want)
        assert fw <= n                                                 # never more forwards than the plain loop's 1 + n
        if not stream:
            assert fw == 1 + st[0] and st[1] >= st[2]
        eos = int(want[n // 2])
        stop = int(np.flatnonzero(want == eos)[0])
        rc, got, _, _ = lookup(stream, eos=eos)
        assert rc == 0 and np.array_equal(got, want[:stop])
    rc, _, _, _ = lookup(0, temperature=0.8)
    assert rc == -10 and b"greedy only" in host.flh_last_error()
    rc, _, _, _ = lookup(1, temperature=0.8)
    assert rc == -10
    host.flh_model_destroy(h)
