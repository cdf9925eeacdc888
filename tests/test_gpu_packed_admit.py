"""StreamBatcher with PackedAdmit (fastllm_host.hpp, through host_capi): the requests admitted in one step share fl_batch_prefill
calls.  fp32, token positions: every request's tokens are EXACTLY those of the batcher that admits with single forwards.  Both
paths stay within 1e-3 of the fp32 oracle, so their logits differ by at most 2e-3, and the oracle's smallest top-2 margin along the
42 greedy steps of the seven requests below is 0.060 / 0.015 / 0.039 (llama_a / mistral_a / qwen2_a, absolute logit units; computed
on the CPU): more than 7 x that difference."""
import ctypes as C

import numpy as np
import pytest

import synth
from test_host_mirror import host  # noqa: F401
from test_gpu_host_mirror import BATCH_DONE_CB, BATCH_TOKEN_CB, make

pytestmark = pytest.mark.gpu

LENS = [3, 17, 9, 33, 1, 20, 12]


class Batcher:
    """One batcher kept over several rounds of requests; requests: (prompt, max_tokens, eos)"""

    def __init__(self, host, h, slots, packed, entries=0, min_match=16, chunk=4, max_seq=96, max_prompt=256, max_tokens=2048):
        sz = C.c_size_t
        host.flh_batcher_create_packed.argtypes = [C.c_void_p, sz, sz, sz, sz, sz, C.c_int, sz, sz, C.POINTER(C.c_void_p)]
        host.flh_batcher_packed_stats.argtypes = [C.c_void_p, C.POINTER(sz), C.POINTER(sz)]
        host.flh_batcher_prefix_stats.argtypes = [C.c_void_p, C.POINTER(sz), C.POINTER(sz), C.POINTER(sz)]
        host.flh_batcher_submit.argtypes = [C.c_void_p, C.c_void_p, sz, sz, C.c_float, C.c_int64, BATCH_TOKEN_CB, BATCH_DONE_CB, C.c_void_p,
                                            C.POINTER(C.c_uint64)]
        host.flh_batcher_run.argtypes = [C.c_void_p, C.POINTER(sz), C.POINTER(sz)]
        host.flh_batcher_destroy.argtypes = [C.c_void_p]
        self.host, self.b, self.got, self.done = host, C.c_void_p(), {}, {}
        assert host.flh_batcher_create_packed(h, slots, max_seq, chunk, entries, min_match, 1 if packed else 0, max_prompt, max_tokens,
                                              C.byref(self.b)) == 0, host.flh_last_error()
        self.cb = BATCH_TOKEN_CB(lambda rid, tok, _u: self.got[rid].append(int(tok)) or 1)
        self.dcb = BATCH_DONE_CB(lambda rid, n, _u: self.done.__setitem__(rid, int(n)))

    def round(self, requests):
        ids = []
        for prompt, max_tokens, eos in requests:
            a = np.ascontiguousarray(prompt, dtype=np.uint32)
            rid = C.c_uint64(0)
            assert self.host.flh_batcher_submit(self.b, a.ctypes.data, a.size, max_tokens, 0.0, eos, self.cb, self.dcb, None, C.byref(rid)) == 0, \
                self.host.flh_last_error()
            self.got[rid.value] = []
            ids.append(rid.value)
        steps, pre = C.c_size_t(0), C.c_size_t(0)
        assert self.host.flh_batcher_run(self.b, C.byref(steps), C.byref(pre)) == 0, self.host.flh_last_error()
        for r in ids:
            assert self.done.get(r) == len(self.got[r]), "request %d: done callback %s, tokens %d" % (r, self.done.get(r), len(self.got[r]))
        self.prefills = pre.value
        return [list(self.got[r]) for r in ids]

    def stats(self):
        a, b, c, d, e = (C.c_size_t(0) for _ in range(5))
        assert self.host.flh_batcher_prefix_stats(self.b, C.byref(a), C.byref(b), C.byref(c)) == 0
        assert self.host.flh_batcher_packed_stats(self.b, C.byref(d), C.byref(e)) == 0
        return dict(prefix_hits=a.value, prefix_tokens_reused=b.value, prefill_tokens=c.value, prefill_calls=d.value, packed_calls=e.value,
                    prefills=self.prefills)

    def close(self):
        self.host.flh_batcher_destroy(self.b)


def one_round(host, h, requests, packed, **kw):
    b = Batcher(host, h, 3, packed, **kw)
    toks = b.round(requests)
    st = b.stats()
    b.close()
    return toks, st


@pytest.mark.parametrize("name", ["llama_a", "mistral_a", "qwen2_a"])
def test_packed_admission_emits_the_tokens_of_single_admission(host, name, monkeypatch):
    monkeypatch.setenv("FASTLLM_POS_MODE", "tokens")
    monkeypatch.setenv("FASTLLM_MAX_SEQ", "96")
    h, cfg, _w = make(host, name, dtype=0)
    reqs = [(synth.prompt_ids(cfg, n, seed=500 + i), 6, -1) for i, n in enumerate(LENS)]
    off, st0 = one_round(host, h, reqs, False)
    on, st1 = one_round(host, h, reqs, True)
    assert all(len(t) == 6 for t in off)
    assert on == off
    assert st0["packed_calls"] == 0 and st0["prefill_calls"] == st0["prefills"] == 7
    assert st1["prefills"] == 7 and st1["prefill_tokens"] == st0["prefill_tokens"] == sum(LENS)
    assert st1["packed_calls"] >= 1 and st1["prefill_calls"] < st0["prefill_calls"]
    # prompts above max_prompt keep the single call: the 33- and 20-token ones here
    on2, st2 = one_round(host, h, reqs, True, max_prompt=17)
    assert on2 == off and st2["prefill_calls"] - st2["packed_calls"] == 2 and st2["prefill_tokens"] == sum(LENS)
    # a call holds at most max_tokens tokens: 3 + 17 | 9 in the first step
    on3, st3 = one_round(host, h, reqs, True, max_tokens=24)
    assert on3 == off and st3["packed_calls"] > st1["packed_calls"]
    host.flh_model_destroy(h)


@pytest.mark.parametrize("name", ["llama_a", "mistral_a", "qwen2_a"])
def test_packed_admission_with_a_prefix_store(host, name, monkeypatch):
    """two rounds of three conversations: the second round's prompts extend the first's and their replies, the suffixes are packed"""
    monkeypatch.setenv("FASTLLM_POS_MODE", "tokens")
    monkeypatch.setenv("FASTLLM_MAX_SEQ", "96")
    h, cfg, _w = make(host, name, dtype=0)
    out = {}
    for packed in (False, True):
        b = Batcher(host, h, 3, packed, entries=4)
        prompts = [synth.prompt_ids(cfg, 20 + c, seed=300 + c).tolist() for c in range(3)]
        toks = []
        for r in range(2):
            replies = b.round([(p, 6, -1) for p in prompts])
            toks += replies
            prompts = [p + rep + synth.prompt_ids(cfg, 5, seed=400 + 10 * r + c).tolist() for c, (p, rep) in enumerate(zip(prompts, replies))]
        out[packed] = (toks, b.stats())
        b.close()
    (t0, s0), (t1, s1) = out[False], out[True]
    assert t1 == t0
    assert s1["prefix_hits"] == s0["prefix_hits"] == 3 and s1["prefix_tokens_reused"] == s0["prefix_tokens_reused"]
    assert s1["prefill_tokens"] == s0["prefill_tokens"]
    assert s1["packed_calls"] >= 2 and s1["prefill_calls"] < s0["prefill_calls"]
    host.flh_model_destroy(h)


def test_packed_admission_finishes_requests_at_their_first_token(host, monkeypatch):
    """max_tokens = 0, and a first token that is the request's EOS: finished inside the admission, their slots go to waiting requests"""
    monkeypatch.setenv("FASTLLM_POS_MODE", "tokens")
    monkeypatch.setenv("FASTLLM_MAX_SEQ", "96")
    h, cfg, _w = make(host, "llama_a", dtype=0)
    reqs = [[synth.prompt_ids(cfg, n, seed=500 + i), 6, -1] for i, n in enumerate(LENS)]
    plain, _ = one_round(host, h, [tuple(r) for r in reqs], False)
    reqs[1][1] = 0                                             # nothing wanted
    reqs[2][2] = plain[2][0]                                   # its first token is its EOS
    reqs[5][2] = plain[5][2]                                   # ... and one that ends a few tokens in
    off, st0 = one_round(host, h, [tuple(r) for r in reqs], False)
    on, st1 = one_round(host, h, [tuple(r) for r in reqs], True)
    assert off[1] == [] and off[2] == [] and off[5] == plain[5][:plain[5].index(plain[5][2])] and off[0] == plain[0]
    assert on == off
    assert st1["prefills"] == st0["prefills"] == 7 and st1["prefill_tokens"] == st0["prefill_tokens"]
    assert st1["packed_calls"] >= 1
    host.flh_model_destroy(h)
