"""StreamBatcher with a PrefixStore (fastllm_host.hpp, through host_capi): chat turns whose prompts extend the previous prompt and
its reply are served from cached K/V -- the tokens are those of the batcher without a store, with fewer prompt tokens forwarded."""
import ctypes as C

import numpy as np
import pytest

import synth
from test_host_mirror import host  # noqa: F401
from test_gpu_host_mirror import BATCH_DONE_CB, BATCH_TOKEN_CB, make

pytestmark = pytest.mark.gpu


class Batcher:
    """One batcher kept over several rounds of requests (its store lives as long as it does)."""

    def __init__(self, host, h, slots, entries, min_match=16, chunk=4, max_seq=96):
        host.flh_batcher_create_prefix.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t, C.POINTER(C.c_void_p)]
        host.flh_batcher_prefix_stats.argtypes = [C.c_void_p, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
        host.flh_batcher_submit.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_float, C.c_int64, BATCH_TOKEN_CB, BATCH_DONE_CB,
                                            C.c_void_p, C.POINTER(C.c_uint64)]
        host.flh_batcher_run.argtypes = [C.c_void_p, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
        host.flh_batcher_destroy.argtypes = [C.c_void_p]
        self.host, self.b, self.got = host, C.c_void_p(), {}
        self.rc = host.flh_batcher_create_prefix(h, slots, max_seq, chunk, entries, min_match, C.byref(self.b))
        self.cb = BATCH_TOKEN_CB(lambda rid, tok, _u: self.got[rid].append(int(tok)) or 1)
        self.dcb = BATCH_DONE_CB(lambda rid, n, _u: None)

    def round(self, prompts, max_tokens):
        ids = []
        for p in prompts:
            a = np.ascontiguousarray(p, dtype=np.uint32)
            rid = C.c_uint64(0)
            assert self.host.flh_batcher_submit(self.b, a.ctypes.data, a.size, max_tokens, 0.0, -1, self.cb, self.dcb, None, C.byref(rid)) == 0, \
                self.host.flh_last_error()
            self.got[rid.value] = []
            ids.append(rid.value)
        steps, pre = C.c_size_t(0), C.c_size_t(0)
        assert self.host.flh_batcher_run(self.b, C.byref(steps), C.byref(pre)) == 0, self.host.flh_last_error()
        return [list(self.got[r]) for r in ids]

    def stats(self):
        a, b, c = C.c_size_t(0), C.c_size_t(0), C.c_size_t(0)
        assert self.host.flh_batcher_prefix_stats(self.b, C.byref(a), C.byref(b), C.byref(c)) == 0
        return dict(prefix_hits=a.value, prefix_tokens_reused=b.value, prefill_tokens=c.value)

    def close(self):
        self.host.flh_batcher_destroy(self.b)


def conversations(host, h, cfg, entries, n_conv, rounds, first_len, turn_len, reply_len, slots=2):
    """`n_conv` conversations of `rounds` turns each: every prompt is the previous prompt, its reply and turn_len new ids.
    Returns (every request's tokens in submission order, every prompt, the batcher's counters)."""
    b = Batcher(host, h, slots, entries)
    assert b.rc == 0, host.flh_last_error()
    prompts = [synth.prompt_ids(cfg, first_len + c, seed=300 + c).tolist() for c in range(n_conv)]
    all_tokens, all_prompts = [], []
    for r in range(rounds):
        replies = b.round(prompts, reply_len)
        all_tokens += replies
        all_prompts += [list(p) for p in prompts]
        prompts = [p + rep + synth.prompt_ids(cfg, turn_len, seed=400 + 10 * r + c).tolist() for c, (p, rep) in enumerate(zip(prompts, replies))]
    st = b.stats()
    b.close()
    return all_tokens, all_prompts, st


@pytest.mark.parametrize("name", ["llama_a", "mistral_a"])
def test_chat_turns_reuse_their_history_and_emit_the_same_tokens(host, name, monkeypatch):
    """Twelve requests in three conversations through two slots, fp32, token positions."""
    monkeypatch.setenv("FASTLLM_POS_MODE", "tokens")
    monkeypatch.setenv("FASTLLM_MAX_SEQ", "96")
    h, cfg, _w = make(host, name, dtype=0)
    plain, prompts0, st0 = conversations(host, h, cfg, 0, 3, 4, 20, 5, 6)
    reuse, prompts1, st1 = conversations(host, h, cfg, 4, 3, 4, 20, 5, 6)
    assert len(plain) == len(reuse) == 12 and all(len(t) == 6 for t in plain)
    assert prompts0 == prompts1
    assert reuse == plain
    assert st0["prefix_hits"] == 0 and st0["prefix_tokens_reused"] == 0
    assert st0["prefill_tokens"] == sum(len(p) for p in prompts0)
    # every turn after a conversation's first finds its previous prompt and all of the reply but its last token
    assert st1["prefix_hits"] == 9
    assert st1["prefix_tokens_reused"] == sum(len(p) - 5 - 1 for p in prompts1[3:])
    assert st1["prefill_tokens"] == st0["prefill_tokens"] - st1["prefix_tokens_reused"] < st0["prefill_tokens"]
    host.flh_model_destroy(h)


def test_prompts_past_the_sliding_window_are_not_reused(host, monkeypatch):
    """mistral_win masks beyond 5 keys inside one call: a cached prefix would not be masked, so every prompt is prefilled whole."""
    monkeypatch.setenv("FASTLLM_POS_MODE", "tokens")
    monkeypatch.setenv("FASTLLM_MAX_SEQ", "96")
    h, cfg, _w = make(host, "mistral_win", dtype=0)
    plain, prompts0, st0 = conversations(host, h, cfg, 0, 2, 3, 20, 5, 6)
    reuse, _, st1 = conversations(host, h, cfg, 4, 2, 3, 20, 5, 6)
    assert reuse == plain
    assert st1["prefix_hits"] == 0 and st1["prefill_tokens"] == st0["prefill_tokens"] == sum(len(p) for p in prompts0)
    host.flh_model_destroy(h)


def test_call_counter_positions_refuse_a_store(host, monkeypatch):
    monkeypatch.setenv("FASTLLM_POS_MODE", "reference")
    monkeypatch.setenv("FASTLLM_MAX_SEQ", "96")
    h, _cfg, _w = make(host, "mistral_a", dtype=0)
    b = Batcher(host, h, 2, 4)
    assert b.rc == -8 and b"token positions" in host.flh_last_error()
    b0 = Batcher(host, h, 2, 0)                       # without a store the call-counter mode is served as before
    assert b0.rc == 0
    b0.close()
    host.flh_model_destroy(h)
