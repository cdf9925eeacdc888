"""StreamBatcher with BatchLookup (fastllm_host.hpp, through host_capi): a step with drafts is ONE fl_batch_verify over the active slots.

fp32, token positions.  Six requests go through three slots: different prompt lengths, max_tokens, temperatures and EOS ids, one
request whose prompt repeats itself and one with logit rules (while it is active every step is the plain chunk).  Drafts come from the
prompts and from the cycles greedy streams of random weights fall into; how many of them are right depends on the model (measured:
llama_a 13 of 43, mistral_a 0 of 11, qwen2_a 7 of 59 accepted), so the test asks for verify steps and drafts, not for acceptance.  With the option on every stream's tokens are those of the batcher with it off: a verify step's rows are the
decode steps' rows up to fp32 summation order, ArgMax rows are selected by the same rule and sampled rows with the word of the token's
index.  With the option off the batcher is the one flh_batcher_create_on makes: the same tokens, the same counters."""
import ctypes as C

import numpy as np
import pytest

import synth
from test_gpu_host_mirror import BATCH_DONE_CB, BATCH_TOKEN_CB
from test_gpu_logit_rules import PEN, RULE_ARGS, rule_args, two_biases
from test_host_mirror import host  # noqa: F401

pytestmark = pytest.mark.gpu

sz = C.c_size_t


@pytest.fixture(scope="module")
def fa():
    import fastllm_amd
    assert fastllm_amd.device_count() >= 1
    return fastllm_amd


def declare(host):  # noqa: F811
    host.flh_batcher_create_on.argtypes = [C.c_void_p, sz, sz, sz, C.c_int, C.POINTER(C.c_void_p)]
    host.flh_batcher_create_on_lookup.argtypes = [C.c_void_p, sz, sz, sz, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, sz, C.POINTER(C.c_void_p)]
    host.flh_batcher_lookup_stats.argtypes = [C.c_void_p, C.POINTER(sz), C.POINTER(sz), C.POINTER(sz)]
    host.flh_batcher_submit.argtypes = [C.c_void_p, C.c_void_p, sz, sz, C.c_float, C.c_int64, BATCH_TOKEN_CB, BATCH_DONE_CB, C.c_void_p, C.POINTER(C.c_uint64)]
    host.flh_batcher_submit_rules.argtypes = [C.c_void_p, C.c_void_p, sz, sz, C.c_float, C.c_int64] + RULE_ARGS + \
                                             [BATCH_TOKEN_CB, BATCH_DONE_CB, C.c_void_p, C.POINTER(C.c_uint64)]
    host.flh_batcher_run.argtypes = [C.c_void_p, C.POINTER(sz), C.POINTER(sz)]
    host.flh_batcher_destroy.argtypes = [C.c_void_p]
    host.flh_last_error.restype = C.c_char_p


def run(host, gm, requests, mode, slots=3, chunk=4, max_seq=96, max_draft=7, min_drafted=1):  # noqa: F811
    """mode: "parent" (flh_batcher_create_on), "off" / "on" (the new entry with the option off / on); requests: dicts with prompt, n,
    temperature, eos and optionally rules.  Returns (tokens per request, counters)."""
    declare(host)
    b = C.c_void_p()
    if mode == "parent":
        rc = host.flh_batcher_create_on(gm._h, slots, max_seq, chunk, 0, C.byref(b))
    else:
        rc = host.flh_batcher_create_on_lookup(gm._h, slots, max_seq, chunk, 0, 1 if mode == "on" else 0, max_draft, 3, 1, min_drafted, C.byref(b))
    assert rc == 0, host.flh_last_error()
    got, done, keep, rids = {}, {}, [], []
    cb = BATCH_TOKEN_CB(lambda rid, tok, _u: got[rid].append(int(tok)) or 1)
    dcb = BATCH_DONE_CB(lambda rid, n, _u: done.__setitem__(rid, int(n)))
    for r in requests:
        p = np.ascontiguousarray(r["prompt"], dtype=np.uint32)
        rid = C.c_uint64(0)
        if r.get("rules"):
            arrays, args = rule_args(r["rules"])
            keep.append(arrays)
            rc = host.flh_batcher_submit_rules(b, p.ctypes.data, p.size, r["n"], r["temperature"], r["eos"], *args, cb, dcb, None, C.byref(rid))
        else:
            rc = host.flh_batcher_submit(b, p.ctypes.data, p.size, r["n"], r["temperature"], r["eos"], cb, dcb, None, C.byref(rid))
        assert rc == 0, host.flh_last_error()
        got[rid.value] = []
        rids.append(rid.value)
    steps, pre = sz(0), sz(0)
    assert host.flh_batcher_run(b, C.byref(steps), C.byref(pre)) == 0, host.flh_last_error()
    v, d, a = sz(0), sz(0), sz(0)
    assert host.flh_batcher_lookup_stats(b, C.byref(v), C.byref(d), C.byref(a)) == 0
    host.flh_batcher_destroy(b)
    for rid in rids:
        assert done.get(rid) == len(got[rid])
    return [got[rid] for rid in rids], dict(batch_steps=steps.value, prefills=pre.value, verify_steps=v.value, drafted=d.value, accepted=a.value)


def scenario(cfg):
    base = synth.prompt_ids(cfg, 10, seed=71)
    repeating = np.concatenate([base, base[1:], base[1:4]]).astype(np.uint32)      # a prompt that repeats itself
    prompts = [synth.prompt_ids(cfg, 9, seed=60), repeating, synth.prompt_ids(cfg, 5, seed=62), synth.prompt_ids(cfg, 17, seed=63),
               synth.prompt_ids(cfg, 12, seed=64), synth.prompt_ids(cfg, 7, seed=65)]
    ns = [24, 48, 12, 30, 24, 8]
    temps = [0.0, 0.0, 0.8, 0.0, 1.0, 0.0]
    return [dict(prompt=p, n=n, temperature=t, eos=-1) for p, n, t in zip(prompts, ns, temps)]


@pytest.mark.parametrize("name", ["llama_a", "mistral_a", "qwen2_a"])
def test_lookup_batcher_emits_the_tokens_of_the_plain_batcher(fa, host, name):  # noqa: F811
    cfg = synth.CONFIGS[name]
    gm = fa.Model(cfg, synth.synth_weights(cfg), dtype="f32")
    reqs = scenario(cfg)
    free, _ = run(host, gm, reqs, "parent")                                # no EOS, no rules: where the streams go on their own
    assert [len(t) for t in free] == [r["n"] for r in reqs]
    # EOS ids out of the streams' own tokens (first occurrences, past the start / the middle), and rules that change the last
    # request's tokens: it is admitted last and is short, so the other streams run with and without a ruled neighbour
    eosed, ruled = (0, 2, 4), 5
    for i, k0 in zip(eosed, (3, 6, 12)):
        k = next(k for k in range(k0, len(free[i])) if free[i][k] not in free[i][:k])
        reqs[i]["eos"] = int(free[i][k])
    reqs[ruled]["rules"] = dict(PEN, logit_bias=two_biases(free[ruled][1]))
    parent, pst = run(host, gm, reqs, "parent")
    off, ost = run(host, gm, reqs, "off")
    on, nst = run(host, gm, reqs, "on")
    assert [len(parent[i]) for i in eosed] == [free[i].index(reqs[i]["eos"]) for i in eosed]             # each stopped at its EOS, which is not emitted
    assert parent[ruled] != free[ruled]
    # off: the parent's batcher -- tokens and every counter
    assert off == parent and ost == pst and ost["verify_steps"] == ost["drafted"] == ost["accepted"] == 0
    # on: the same tokens per stream, through verify steps
    for i, (a, b) in enumerate(zip(on, parent)):
        assert a == b, "request %d" % i
    print("%s: %s" % (name, nst))
    assert nst["verify_steps"] > 0 and nst["accepted"] <= nst["drafted"] and nst["drafted"] > 0 and nst["prefills"] == pst["prefills"] == len(reqs)
    assert nst["batch_steps"] > 0                                           # the ruled request forced plain chunks while it was active
    # min_drafted above anything a step can draft: every step is the plain chunk again
    never, vst = run(host, gm, reqs, "on", min_drafted=10 ** 6)
    assert never == parent and vst == pst
    gm.close()


def test_lookup_batcher_refuses_counter_positions(fa, host):  # noqa: F811
    cfg = synth.CONFIGS["mistral_a"]
    gm = fa.Model(cfg, synth.synth_weights(cfg), dtype="f32")
    declare(host)
    b = C.c_void_p()
    assert host.flh_batcher_create_on_lookup(gm._h, 2, 96, 4, 1, 1, 7, 3, 1, 1, C.byref(b)) == -8
    assert b"token positions" in host.flh_last_error() and not b.value
    assert host.flh_batcher_create_on_lookup(gm._h, 2, 96, 4, 0, 1, 16, 3, 1, 1, C.byref(b)) == -8        # the lookup options' own range error
    assert b"max_draft" in host.flh_last_error() and not b.value
    assert host.flh_batcher_create_on_lookup(gm._h, 2, 96, 4, 1, 0, 7, 3, 1, 1, C.byref(b)) == 0          # off: counter positions are the parent's business
    host.flh_batcher_destroy(b)
    gm.close()
