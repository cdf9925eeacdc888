"""Prompt log-probabilities through the model (fl_forward_score): every row of a forward scored on the device.

  1. the records are the scores of the rows the kernel read (logits_out): lc.check_row + the exact rank, any dtype;
  2. those rows are the forward's: bit for bit the rows a verify step returns for the same ids (same path, same launch shapes);
  3. / 4. fp32 against the oracle, with the forward chunked and lm_head in blocks of 8 rows; behind a cached prefix;
  5. a scored cache is the forwarded cache;  6. T = 1 is the decode step;  7. nothing else launches anything new;
  8. the refusals;  9. the C++ host mirror's score_ids."""
import ctypes as C

import numpy as np
import pytest

import score_cases as sc
import synth
from oracle import oracle
from score_cases import lc
from test_host_mirror import host  # noqa: F401

pytestmark = pytest.mark.gpu
CAP = 96
NO = sc.NO_TARGET
LOGIT_BAR = 2e-3          # twice the fp32 mode's project bar on logits against the oracle (tests/test_gpu_parity.py: 1e-3): x_t and the row move apart by at most that


@pytest.fixture(scope="module")
def fa():
    import fastllm_amd
    assert fastllm_amd.device_count() >= 1
    return fastllm_amd


class Models:
    """(GPU model, config) of a config and dtype, built once per module and CLOSED with it: a model left alive would keep its stream,
    and later modules that need the device's hardware queues to themselves (tests/test_gpu_tp_ipc.py) must not meet it."""

    def __init__(self, fa):
        self.fa, self.built = fa, {}

    def get(self, name, dtype):
        if (name, dtype) not in self.built:
            cfg = synth.CONFIGS[name]
            self.built[(name, dtype)] = (self.fa.Model(cfg, synth.synth_weights(cfg), dtype=dtype), cfg)
        return self.built[(name, dtype)]

    def close(self):
        for gm, _ in self.built.values():
            gm.close()
        self.built.clear()


@pytest.fixture(scope="module")
def models(fa):
    m = Models(fa)
    yield m
    m.close()


_oracles = {}


def oracle_model(name):
    if name not in _oracles:
        cfg = synth.CONFIGS[name]
        _oracles[name] = oracle.OracleModel(cfg, synth.as_f32(synth.synth_weights(cfg)), round_bf16=False)
    return _oracles[name]


@pytest.fixture(scope="module", params=["bf16", "f32"])
def env(models, request):
    gm, cfg = models.get("llama_a", request.param)
    return gm, cfg, request.param


def check_against_rows(res, rows, targets, top_n, what):
    assert res.target_logprob.shape == (len(targets),) and res.top_ids.shape == (len(targets), top_n)
    for t, g in enumerate(targets):
        sc.check_scored_row(rows[t], g, top_n, res, t, what=what)


def check_against_oracle(res, orows, targets, top_n, what):
    """Every row against the oracle's row (fp32 mode): the bound follows from the 1e-3 bar on logits, see the module docstring of
    tests/test_gpu_parity.py -- |dlp| <= 2e-3 + lc.tol; the rank inside the interval the bar leaves open; the reported top ids
    descending on the oracle row within 2e-3, each at least the top_n-th largest - 2e-3."""
    for t, g in enumerate(targets):
        x = np.asarray(orows[t], dtype=np.float32)
        lp, order = lc.ref_logprobs(x)
        tol = LOGIT_BAR + lc.tol(x, lp)
        if int(g) == NO:
            assert np.isnan(res.target_logprob[t]) and int(res.target_rank[t]) == 0, (what, t)
        else:
            g = int(g)
            assert abs(float(res.target_logprob[t]) - lp[g]) <= tol[g], (what, t, float(res.target_logprob[t]), lp[g], tol[g])
            lo, hi = 1 + int((x > x[g] + LOGIT_BAR).sum()), int((x >= x[g] - LOGIT_BAR).sum())
            assert lo <= int(res.target_rank[t]) <= hi, (what, t, int(res.target_rank[t]), lo, hi)
        ids = res.top_ids[t].astype(np.int64)
        assert len(set(ids.tolist())) == top_n and (ids < x.size).all(), (what, t)
        if top_n:
            v = x[ids]
            assert (v[:-1] >= v[1:] - LOGIT_BAR).all(), (what, t, "order", v)
            assert (v >= x[order[top_n - 1]] - LOGIT_BAR).all(), (what, t, "membership", v)
            for j, i in enumerate(ids):
                assert abs(float(res.top_logprobs[t][j]) - lp[i]) <= tol[i], (what, t, j)


def oracle_rows(om, prefix, rest):
    """Row i of `rest` behind the cached `prefix`: the last row of forward(prefix) (if any) then forward(rest[:i + 1]) on a fresh cache
    -- exact for causal and windowed masks"""
    out = []
    for i in range(len(rest)):
        c = om.new_cache(CAP)
        if len(prefix):
            om.forward(c, prefix, 0)
        out.append(np.array(om.forward(c, rest[:i + 1], len(prefix)), dtype=np.float32))
    return out


# ---- 1. the rows the kernel read
@pytest.mark.parametrize("T", [2, 23])
def test_records_are_the_scores_of_the_returned_rows(env, T):
    gm, cfg, dtype = env
    V = cfg["vocab_size"]
    ids = synth.prompt_ids(cfg, T, seed=31)
    rs = np.random.RandomState(5)
    explicit = rs.randint(0, V, T).astype(np.uint32)
    mixed = explicit.copy()
    mixed[::3] = NO
    for targets, want in ((None, sc.next_targets(ids)), (explicit, explicit), (mixed, mixed)):
        for top_n in (0, 5):
            c = gm.new_cache(CAP)
            res = gm.forward_score(c, ids, 0, top_n=top_n, targets=targets, want_logits=True)
            assert res.logits.shape == (T, V) and len(c) == T
            check_against_rows(res, res.logits, want, top_n, (dtype, T, top_n))
            plain = gm.forward_score(gm.new_cache(CAP), ids, 0, top_n=top_n, targets=targets)
            assert plain.logits is None
            for a, b in zip(plain[:4], res[:4]):                        # (the diagnostic copy changes nothing)
                assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert np.isnan(gm.forward_score(gm.new_cache(CAP), ids, 0).target_logprob[-1])


# ---- 2. those rows are the forward's
@pytest.mark.parametrize("T", [2, 9, 16])
def test_rows_are_the_verify_steps_rows(env, T):
    gm, cfg, dtype = env
    ids = synth.prompt_ids(cfg, T, seed=32)
    a, b = gm.new_cache(CAP), gm.new_cache(CAP)
    res = gm.forward_score(a, ids, 0, want_logits=True)
    _, lg = gm.forward_verify(b, ids[0], ids[1:], 0, want_logits=True)
    assert lg.shape == res.logits.shape and np.array_equal(lg.view(np.uint32), res.logits.view(np.uint32))


# ---- 3. against the oracle, chunking forced
@pytest.mark.parametrize("name", ["llama_a", "qwen2_a", "mistral_win", "qwen2_win"])
def test_fp32_against_the_oracle_chunked(fa, models, name):
    gm, cfg = models.get(name, "f32")                                    # (built before the switches are lowered)
    om = oracle_model(name)
    T, top_n = 40, 5
    ids = synth.prompt_ids(cfg, T, seed=33)
    orows = oracle_rows(om, ids[:0], ids)
    try:
        fa.tune("score_rows", 8)                                        # lm_head blocks of 8 rows: 2 per forward chunk of 16, 1 for the last 8
        fa.tune("prefill_chunk", 16)                                    # forward chunks of 16 / 16 / 8
        c = gm.new_cache(CAP)
        res = gm.forward_score(c, ids, 0, top_n=top_n, want_logits=True)
    finally:
        fa.reload_env()
    assert len(c) == T
    check_against_oracle(res, orows, sc.next_targets(ids), top_n, name)
    check_against_rows(res, res.logits, sc.next_targets(ids), top_n, name)
    for t in range(T):
        assert np.abs(res.logits[t] - orows[t]).max() <= 1e-3, (name, t)


# ---- 4. behind a cached prefix
@pytest.mark.parametrize("name", ["llama_a", "qwen2_a"])
def test_fp32_cached_prefix(models, name):
    gm, cfg = models.get(name, "f32")
    om = oracle_model(name)
    ids = synth.prompt_ids(cfg, 32, seed=34)
    prefix, rest = ids[:12], ids[12:]
    c = gm.new_cache(CAP)
    gm.forward(c, prefix, 0)
    res = gm.forward_score(c, rest, 12, top_n=3)
    assert len(c) == 32
    check_against_oracle(res, oracle_rows(om, prefix, rest), sc.next_targets(rest), 3, name)


# ---- 5. a scored cache is the forwarded cache
def test_scored_cache_is_the_forwarded_cache(env):
    gm, cfg, dtype = env
    ids = synth.prompt_ids(cfg, 21, seed=35)
    a, b = gm.new_cache(CAP), gm.new_cache(CAP)
    gm.forward_score(a, ids, 0, top_n=2)
    first = oracle.argmax(gm.forward(b, ids, 0))
    assert len(a) == len(b) == 21
    assert np.array_equal(gm.decode_greedy(a, first, 21, 8), gm.decode_greedy(b, first, 21, 8))


# ---- 6. T = 1
def test_single_token_takes_the_decode_step(env):
    gm, cfg, dtype = env
    ids = synth.prompt_ids(cfg, 9, seed=36)
    a, twin = gm.new_cache(CAP), gm.new_cache(CAP)
    gm.forward(a, ids[:8], 0), gm.forward(twin, ids[:8], 0)
    for s, g in enumerate((5, NO, 7)):                                  # (three calls: the twin's decode graph is captured on the way)
        tok = [(int(ids[8]) + s) % cfg["vocab_size"]]
        res = gm.forward_score(a, tok, 8 + s, top_n=20, targets=[g], want_logits=True)
        row = gm.forward(twin, tok, 8 + s)
        assert np.array_equal(row.view(np.uint32), res.logits[0].view(np.uint32)) and len(a) == len(twin) == 9 + s
        check_against_rows(res, [row], [g], 20, ("T = 1", s))
    res = gm.forward_score(a, [1], 11)                                  # default targets of one row: none
    assert np.isnan(res.target_logprob[0]) and int(res.target_rank[0]) == 0


# ---- 7. nothing else moved
def test_other_calls_launch_what_they_launched(env):
    gm, cfg, dtype = env
    ids = synth.prompt_ids(cfg, 24, seed=37)
    names = lambda stats: sorted((s["name"], s["launches"]) for s in stats)

    def plain():
        c = gm.new_cache(CAP)
        gm.profile_begin()
        first = oracle.argmax(gm.forward(c, ids, 0))
        toks = gm.decode_greedy(c, first, 24, 4)
        return names(gm.profile_end()), toks

    before, toks0 = plain()
    c = gm.new_cache(CAP)
    gm.profile_begin(); gm.forward_score(c, ids, 0, top_n=5); scored = gm.profile_end()
    after, toks1 = plain()
    assert before == after and np.array_equal(toks0, toks1)
    assert sum(s["launches"] for s in scored if "[score]" in s["name"]) == 1
    assert not [n for n, _ in before if "score" in n]


# ---- 8. refusals
def test_refusals(fa, models):
    cfg = synth.CONFIGS["llama_a"]
    ids = synth.prompt_ids(cfg, 8, seed=38)
    gm2 = fa.Model(cfg, synth.synth_weights(cfg), dtype="bf16", tp_mode=fa.binding.TP_EMULATED, tp_size=2)
    c = gm2.new_cache(CAP)
    with pytest.raises(fa.FastLLMError) as e:
        gm2.forward_score(c, ids, 0)
    assert e.value.code == -10 and len(c) == 0
    c.close(); gm2.close()
    gm, _ = models.get("llama_a", "bf16")
    c = gm.new_cache(16)
    gm.forward(c, ids, 0)
    with pytest.raises(fa.FastLLMError) as e:
        gm.forward_score(c, synth.prompt_ids(cfg, 9, seed=39), 8)
    assert e.value.code == -7 and len(c) == 8
    with pytest.raises(fa.FastLLMError) as e:                           # a target outside the vocabulary names the field
        gm.forward_score(c, ids[:4], 8, targets=[0, cfg["vocab_size"], NO, 1])
    assert e.value.code == -8 and "targets" in str(e.value) and len(c) == 8
    res = gm.forward_score(c, ids[:4], 8, targets=[0, cfg["vocab_size"] - 1, NO, 1])
    assert len(c) == 12 and np.isnan(res.target_logprob[2])


# ---- 9. the host mirror
def test_host_mirror_score_ids(fa, host, monkeypatch):  # noqa: F811
    from test_gpu_host_mirror import make
    monkeypatch.setenv("FASTLLM_POS_MODE", "tokens")
    monkeypatch.setenv("FASTLLM_MAX_SEQ", "64")
    host.flh_score_ids.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    h, cfg, w = make(host, "llama_a", dtype=0)
    ids = np.ascontiguousarray(synth.prompt_ids(cfg, 19, seed=40), dtype=np.uint32)
    lp, rank = np.zeros(19, np.float32), np.zeros(19, np.uint32)
    top_ids, top = np.zeros((19, 3), np.uint32), np.zeros((19, 3), np.float32)
    rc = host.flh_score_ids(h, ids.ctypes.data, ids.size, 3, lp.ctypes.data, rank.ctypes.data, top_ids.ctypes.data, top.ctypes.data)
    assert rc == 0, host.flh_last_error()
    gm = fa.Model(cfg, w, dtype="f32")
    res = gm.forward_score(gm.new_cache(64), ids, 0, top_n=3)
    assert np.array_equal(lp.view(np.uint32), res.target_logprob.view(np.uint32)) and np.array_equal(rank, res.target_rank)
    assert np.array_equal(top_ids, res.top_ids) and np.array_equal(top.view(np.uint32), res.top_logprobs.view(np.uint32))
    host.flh_model_destroy(h)
    gm.close()
