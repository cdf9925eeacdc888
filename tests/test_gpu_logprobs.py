"""Token log-probabilities through the model (fl_forward_sample_lp, fl_decode_sample_lp, fl_batch_decode_each_lp), bf16 and fp32.
Yardstick for a step: float64 log-softmax of the logits fl_forward (or fl_batch_forward) returns for the same step on a TWIN cache
fed the same ids -- the forward is deterministic, so those rows are the bits the log-prob kernel read.  Values within the derived
tolerance of tests/logprob_cases.py, top ids exactly, tokens identical to the calls without log-probs."""
import ctypes as C

import numpy as np
import pytest

import logprob_cases as lc
import synth
from test_host_mirror import host  # noqa: F401

pytestmark = pytest.mark.gpu
CAP = 96
NP = 8                                       # prompt length
SAMPLERS = [dict(temperature=0.0), dict(temperature=0.8, top_p=0.9, seed=3)]


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


def check_steps(gm, twin, first, pos, toks, rec, top_n, what):
    """rec = (token_logprob, top_ids, top_logprobs) of the steps that emitted toks, against teacher-forced T = 1 forwards on twin."""
    tl, ids, lps = rec
    assert tl.shape == (len(toks),) and ids.shape == (len(toks), top_n) and lps.shape == (len(toks), top_n), what
    for s, t in enumerate(toks):
        row = gm.forward(twin, [first if s == 0 else toks[s - 1]], pos + s)
        lc.check_row(row, t, top_n, tl[s], ids[s], lps[s], what=(what, s))


@pytest.mark.parametrize("sampler", SAMPLERS)
def test_prefill(env, sampler):
    gm, cfg, prompt = env
    a, b, twin = gm.new_cache(CAP), gm.new_cache(CAP), gm.new_cache(CAP)
    want = gm.forward_sample(a, prompt, 0, **sampler)
    tok, tl, ids, lps = gm.forward_sample(b, prompt, 0, logprobs=5, **sampler)
    assert tok == want and len(a) == len(b) == NP
    lc.check_row(gm.forward(twin, prompt, 0), tok, 5, tl[0], ids[0], lps[0], what="prefill")


def test_single_token_forward(env):
    """T = 1 goes through the decode step (and its second graph from the second call on): record 0 of a call of one step."""
    gm, cfg, prompt = env
    (a, first), (twin, _) = prefilled(gm, prompt), prefilled(gm, prompt)
    tok = first
    for s in range(3):
        row = gm.forward(twin, [tok], NP + s)
        nxt, tl, ids, lps = gm.forward_sample(a, [tok], NP + s, 0.0, logprobs=20)
        lc.check_row(row, nxt, 20, tl[0], ids[0], lps[0], what=("T = 1", s))
        assert nxt == int(np.flatnonzero(row == row.max())[-1])
        tok = nxt


@pytest.mark.parametrize("sampler", SAMPLERS)
def test_decode_40_steps_in_two_chunks(env, sampler):
    gm, cfg, prompt = env
    (a, first), (b, _), (twin, _) = prefilled(gm, prompt), prefilled(gm, prompt), prefilled(gm, prompt)
    free = gm.decode_sample(prefilled(gm, prompt)[0], first, NP, 40, **sampler)
    eos = next(i for i in range(cfg["vocab_size"]) if i not in set(free.tolist()) and i != first)      # an id that does not occur: chunks of 16 + 24
    want = gm.decode_sample(a, first, NP, 40, eos=eos, **sampler)
    toks, tl, ids, lps = gm.decode_sample(b, first, NP, 40, eos=eos, logprobs=5, **sampler)
    assert len(want) == 40 and np.array_equal(toks, want) and np.array_equal(want, free) and len(a) == len(b)
    check_steps(gm, twin, first, NP, toks, (tl, ids, lps), 5, "decode")


@pytest.mark.parametrize("sampler", SAMPLERS)
def test_decode_stops_at_eos(env, sampler):
    gm, cfg, prompt = env
    (a, first), (b, _), (c, _), (twin, _) = (prefilled(gm, prompt) for _ in range(4))
    free = gm.decode_sample(a, first, NP, 40, **sampler)
    eos = int(free[9])
    n = int(np.flatnonzero(free == eos)[0])                                  # (9 unless the id came earlier as well)
    want = gm.decode_sample(b, first, NP, 40, eos=eos, **sampler)
    toks, tl, ids, lps = gm.decode_sample(c, first, NP, 40, eos=eos, logprobs=20, **sampler)
    assert len(want) == n and np.array_equal(toks, want) and len(b) == len(c)
    if sampler["temperature"] == 0.0:
        assert n == 9 or eos in free[:9].tolist()
    check_steps(gm, twin, first, NP, toks, (tl, ids, lps), 20, "eos")


def test_alternating_calls_on_one_cache(env):
    gm, cfg, prompt = env
    (a, first), (b, _), (twin, _) = prefilled(gm, prompt), prefilled(gm, prompt), prefilled(gm, prompt)
    want = gm.decode_sample(a, first, NP, 18, 0.0)
    t0, *r0 = gm.decode_sample(b, first, NP, 6, 0.0, logprobs=5)
    t1 = gm.decode_sample(b, t0[-1], NP + 6, 6, 0.0)
    t2, *r2 = gm.decode_sample(b, t1[-1], NP + 12, 6, 0.0, logprobs=20)
    assert np.array_equal(np.concatenate([t0, t1, t2]), want) and len(a) == len(b)
    check_steps(gm, twin, first, NP, t0, r0, 5, "segment 0")
    for s, t in enumerate(t1):
        gm.forward(twin, [t0[-1] if s == 0 else t1[s - 1]], NP + 6 + s)
    check_steps(gm, twin, t1[-1], NP + 12, t2, r2, 20, "segment 2")


def test_sampler_does_not_change_the_distribution(env):
    """The same row reports the same values under ArgMax and under temperature / top-p sampling."""
    gm, cfg, prompt = env
    a, b = gm.new_cache(CAP), gm.new_cache(CAP)
    _, _, i0, l0 = gm.forward_sample(a, prompt, 0, 0.0, logprobs=20)
    _, _, i1, l1 = gm.forward_sample(b, prompt, 0, 0.7, top_p=0.9, seed=11, logprobs=20)
    assert np.array_equal(i0, i1) and np.array_equal(l0, l1)


@pytest.mark.parametrize("B", [2, 3])
def test_batch(fa, env, B):
    gm, cfg, prompt = env
    lens = [NP, 5, 7][:B]
    tops = [0, 3, 20][:B]
    temps, top_p, seeds = [0.0, 0.8, 0.9][:B], [None, 0.9, None][:B], [0, 5, 6][:B]

    def fresh(n):
        c = gm.new_cache(CAP)
        return c, gm.forward_argmax(c, prompt[:n], 0)

    def run(members):
        """12 steps of members (list of (len, top_n, temp, top_p, seed)) with log-probs, without, and teacher-forced."""
        ls = [m[0] for m in members]
        sets = [[fresh(n) for n in ls] for _ in range(3)]
        firsts = [f for _, f in sets[0]]
        ba, bb, bt = (fa.Batch(gm, [c for c, _ in s]) for s in sets)
        kw = dict(temperatures=[m[2] for m in members], top_p=[m[3] for m in members], seeds=[m[4] for m in members])
        want = ba.decode_each(firsts, ls, 12, **kw)
        got = bb.decode_each(firsts, ls, 12, logprobs=[m[1] for m in members], **kw)
        for i in range(len(members)):
            assert np.array_equal(got[i][0], want[i]) and len(want[i]) == 12, i
            assert len(sets[0][i][0]) == len(sets[1][i][0])
        return ls, firsts, got, (ba, bb, bt), sets

    def teacher(bt, ls, firsts, got, tops_, what):
        for s in range(12):
            toks = [firsts[i] if s == 0 else got[i][0][s - 1] for i in range(len(ls))]
            lg, _ = bt.forward(toks, [n + s for n in ls])
            for i in range(len(ls)):
                t, tl, ids, lps = got[i]
                assert ids.shape == (12, tops_[i])
                lc.check_row(lg[i], t[s], tops_[i], tl[s], ids[s], lps[s], what=(what, i, s))

    members = list(zip(lens, tops, temps, top_p, seeds))
    ls, firsts, got, (ba, bb, bt), sets = run(members)
    teacher(bt, ls, firsts, got, tops, "batch")
    # a replaced slot: another stream's cache (which has never been asked for log-probs) joins all three batches
    slot = B - 1
    news = [fresh(6) for _ in range(3)]
    for bat, (c, _) in zip((ba, bb, bt), news):
        bat.replace(slot, c)
    ls2 = [len(sets[0][i][0]) for i in range(B)]
    ls2[slot] = 6
    firsts2 = [int(got[i][0][-1]) for i in range(B)]
    firsts2[slot] = news[0][1]
    kw = dict(temperatures=temps, top_p=top_p, seeds=seeds)
    tops2 = tops[::-1]
    want2 = ba.decode_each(firsts2, ls2, 12, **kw)
    got2 = bb.decode_each(firsts2, ls2, 12, logprobs=tops2, **kw)
    for i in range(B):
        assert np.array_equal(got2[i][0], want2[i]), i
    teacher(bt, ls2, firsts2, got2, tops2, "after replace")


def test_tensor_parallel_is_refused(fa):
    cfg = synth.CONFIGS["llama_a"]
    gm = fa.Model(cfg, synth.synth_weights(cfg), dtype="bf16", tp_mode=fa.binding.TP_EMULATED, tp_size=2)
    prompt = synth.prompt_ids(cfg, NP)
    c = gm.new_cache(CAP)
    with pytest.raises(fa.FastLLMError) as e:
        gm.forward_sample(c, prompt, 0, 0.0, logprobs=3)
    assert e.value.code == -10 and len(c) == 0
    first = gm.forward_argmax(c, prompt, 0)
    with pytest.raises(fa.FastLLMError) as e:
        gm.decode_sample(c, first, NP, 4, 0.0, logprobs=0)
    assert e.value.code == -10 and len(c) == NP
    with pytest.raises(fa.FastLLMError) as e:                          # an argument error stays an argument error
        gm.decode_sample(c, first, NP, 4, 0.0, logprobs=21)
    assert e.value.code == -8 and len(c) == NP


def test_plain_decode_launches_what_it_launched(env):
    """The log-prob launch exists only in the calls that ask for it: a plain decode's kernel list has one selection launch per
    step, a log-prob decode's two (+ the one that writes top_n)."""
    gm, cfg, prompt = env
    c, first = prefilled(gm, prompt)
    count = lambda stats, name="select_advance": sum(s["launches"] for s in stats if s["name"] == name)
    gm.profile_begin(); gm.decode_greedy(c, first, NP, 4); plain = gm.profile_end()
    gm.profile_begin(); gm.decode_sample(c, first, NP + 4, 4, 0.0, logprobs=5); with_lp = gm.profile_end()
    gm.profile_begin(); gm.decode_greedy(c, first, NP + 8, 4); plain2 = gm.profile_end()
    assert count(plain) == 4 and count(plain2) == 4 and count(with_lp) == 4
    assert count(with_lp, "select_advance[logprobs]") == 5 and count(plain, "select_advance[logprobs]") == 0
    names = lambda stats: sorted((s["name"], s["launches"]) for s in stats)
    assert names(plain) == names(plain2)


def test_host_mirror_generate_ids_with_logprobs(fa, host, monkeypatch):  # noqa: F811
    from test_gpu_host_mirror import generate, make
    monkeypatch.setenv("FASTLLM_POS_MODE", "tokens")
    monkeypatch.setenv("FASTLLM_MAX_SEQ", "64")
    host.flh_generate_logprobs.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_float, C.c_int64, C.c_double, C.c_int64, C.c_int,
                                           C.c_void_p, C.POINTER(C.c_size_t), C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_size_t)]
    h, cfg, w = make(host, "llama_a", dtype=0)
    prompt = synth.prompt_ids(cfg, NP)
    want, _ = generate(host, h, prompt, 10)
    p = np.ascontiguousarray(prompt, dtype=np.uint32)
    out, tl = np.zeros(10, np.uint32), np.zeros(10, np.float32)
    ids, lps = np.zeros((10, 3), np.uint32), np.zeros((10, 3), np.float32)
    n, fw = C.c_size_t(0), C.c_size_t(0)
    rc = host.flh_generate_logprobs(h, p.ctypes.data, p.size, 10, 0.0, -1, 0.0, 0, 3, out.ctypes.data, C.byref(n), tl.ctypes.data, ids.ctypes.data,
                                    lps.ctypes.data, C.byref(fw))
    assert rc == 0, host.flh_last_error()
    assert n.value == 10 and np.array_equal(out, want) and fw.value == 10
    gm = fa.Model(cfg, w, dtype="f32")
    c = gm.new_cache(64)
    t0, a0, b0, c0 = gm.forward_sample(c, prompt, 0, 0.0, logprobs=3)
    t1, a1, b1, c1 = gm.decode_sample(c, t0, NP, 9, 0.0, logprobs=3)
    assert np.array_equal(out, np.concatenate([[t0], t1]))
    assert np.array_equal(tl, np.concatenate([a0, a1])) and np.array_equal(ids, np.concatenate([b0, b1])) and np.array_equal(lps, np.concatenate([c0, c1]))
    host.flh_model_destroy(h)
