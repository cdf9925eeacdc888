"""Packed verify for full requests through the C ABI (fl_batch_verify_lp, fl_batch_decode_lookup_lp): one pack of four members -- bare,
ruled, guided, ruled + guided -- on the cases of test_gpu_verify_lp.py (models, prompt seeds, rules, automaton, helpers).

  1. the packed step is an exact function of its own logits_out: adjust (verify_adjust_ref.py), ArgMax or fl_op_sample_ex, accept
     reproduce every member's ids, its table afterwards and its guide state, without tolerance, in both dtypes; drafts of 0, 3, 15, 15;
  2. log-probs (top_n 5 / none / 0 / 3 per member) are the float64 log-softmax of the RAW row of each returned id
     (logprob_cases.check_row, its tolerance);
  3. a bare pack with lps = NULL is fl_batch_verify bit for bit;
  4. fp32, per member: ids, table and guide state of fl_forward_verify_lp on a cache of its own;
  5. fp32, the loop per member: the ids, table, guide state and length of fl_decode_lookup_lp on its own cache, with an EOS inside an
     accepted run for the ruled + guided member;
  6. refusals modify nothing and zero n_out;
  7. the host mirror's StreamBatcher with BatchLookup on and a guided slot active takes verify steps and emits the ids of the same
     batcher with the option off."""
import ctypes as C

import numpy as np
import pytest

import logprob_cases as lc
import synth
import verify_adjust_ref as va
from test_gpu_verify_lp import GREEDY, TOPP, fa, half_right, model, plain_loop, selector, start, state_of  # noqa: F401
from test_host_mirror import host  # noqa: F401
from test_verify_lp_margin import EOS_AT, L, Teacher, automaton_of

pytestmark = pytest.mark.gpu

NAMES = ["llama_a", "mistral_a", "qwen2_a"]
PACK_FORMS = ["none", "rules", "guide", "both"]
N_DRAFT = [0, 3, 15, 15]
SPS = [GREEDY, TOPP, GREEDY, TOPP]
TOP_NS = [5, None, 0, 3]
BAD_ARGUMENT = -8          # FL_ERR_BAD_ARGUMENT


def pack(fa, name, dtype, forms=PACK_FORMS, sps=SPS):
    """every member's fresh cache, teacher, first token and half-right draft"""
    cfg = synth.CONFIGS[name]
    out = []
    for form, sp, nd in zip(forms, sps, N_DRAFT):
        _, first, cont, _, _, _ = plain_loop(fa, name, dtype, form, sp, 15)
        c, p, _ = start(fa, name, dtype, form)
        out.append((c, Teacher(cfg, p, form), first, half_right(cfg, cont, nd)))
    return out


def sampler_lists(sps):
    return dict(temperatures=[sp["temperature"] or None for sp in sps], seeds=[sp["seed"] for sp in sps], top_p=[sp["top_p"] for sp in sps],
                draws_done=[1] * len(sps))


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("name", NAMES)
def test_packed_step_is_an_exact_function_of_its_own_logits(fa, name, dtype):
    gm = model(fa, name, dtype)
    mem = pack(fa, name, dtype)
    toks, lg, lps = gm.verify_packed_lp([m[0] for m in mem], [m[2] for m in mem], [m[3] for m in mem], [L] * 4, logprobs=TOP_NS,
                                        want_logits=True, **sampler_lists(SPS))
    off = np.concatenate([[0], np.cumsum([len(m[3]) + 1 for m in mem])])
    for i, (c, t, first, draft) in enumerate(mem):
        case = (name, dtype, PACK_FORMS[i])
        cut = t.cut(draft)
        inputs = [first] + cut
        raw = lg[off[i]: off[i] + len(inputs)]
        want = va.accept(t.rows(raw, inputs), cut, selector(fa, SPS[i], 1))
        assert toks[i].tolist() == want, (case, toks[i].tolist(), want)
        assert len(c) == L + len(want), case
        if t.words is not None:
            assert np.array_equal(c.logit_counts(), va.count_rows(t.words, inputs, len(want))), case
        if t.auto is not None:
            assert c.guide_state() == t.auto.walk_all(0, want), case
        if TOP_NS[i] is None:
            assert lps[i] is None
            continue
        tlp, ids, top = lps[i]
        for k, tok in enumerate(want):
            lc.check_row(raw[k], tok, TOP_NS[i], tlp[k], ids[k], top[k], what=str(case + (k,)))


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_bare_pack_is_batch_verify(fa, dtype):
    gm = model(fa, "llama_a", dtype)
    res = []
    for call in (lambda *a, **k: gm.verify_packed_lp(*a, **k)[:2], gm.verify_packed):
        mem = pack(fa, "llama_a", dtype, forms=["none"] * 4)
        got, lg = call([m[0] for m in mem], [m[2] for m in mem], [m[3] for m in mem], [L] * 4, want_logits=True, **sampler_lists(SPS))
        res.append((got, lg, [len(m[0]) for m in mem]))
    (ga, la, na), (gb, lb, nb) = res
    assert all(np.array_equal(x, y) for x, y in zip(ga, gb)) and na == nb and np.array_equal(la.view(np.uint32), lb.view(np.uint32))


@pytest.mark.parametrize("name", NAMES)
def test_member_equals_forward_verify_lp(fa, name):
    gm = model(fa, name, "f32")
    mem = pack(fa, name, "f32")
    toks, _, _ = gm.verify_packed_lp([m[0] for m in mem], [m[2] for m in mem], [m[3] for m in mem], [L] * 4, **sampler_lists(SPS))
    for i, (c, t, first, draft) in enumerate(mem):
        own, _, _ = start(fa, name, "f32", PACK_FORMS[i])
        sp = SPS[i]
        want, _ = gm.forward_verify_lp(own, first, draft, L, temperature=sp["temperature"], top_p=sp["top_p"], seed=sp["seed"], draws_done=1)
        assert np.array_equal(toks[i], want), (name, PACK_FORMS[i], toks[i], want)
        a, b = state_of(c, PACK_FORMS[i]), state_of(own, PACK_FORMS[i])
        assert (a[0] is None or np.array_equal(a[0], b[0])) and a[1:] == b[1:], (name, PACK_FORMS[i])


@pytest.mark.parametrize("name", NAMES)
def test_loop_equals_decode_lookup_lp(fa, name):
    gm = model(fa, name, "f32")
    n_steps, caches, owns, corpora, firsts, eos = 24, [], [], [], [], []
    for form in PACK_FORMS:
        _, first, cont, _, _, _ = plain_loop(fa, name, "f32", form, GREEDY, n_steps)
        caches.append(start(fa, name, "f32", form)[0])
        owns.append(start(fa, name, "f32", form)[0])
        corpora.append(np.asarray(cont, np.uint32))
        firsts.append(first)
        eos.append(int(cont[EOS_AT]) if form == "both" else -1)      # (test_verify_lp_margin.eos_case: the id's first occurrence)
    got, lps, stats = gm.decode_lookup_packed_lp(caches, corpora, firsts, [L] * 4, [n_steps] * 4, eos=eos, logprobs=[None, 2, None, 2])
    for i, form in enumerate(PACK_FORMS):
        want, wlp, _, _, wst = gm.decode_lookup_lp(owns[i], corpora[i], firsts[i], L, n_steps, eos=eos[i], logprobs=2, return_stats=True)
        assert np.array_equal(got[i], want), (name, form, got[i], want)
        assert len(want) == (EOS_AT if form == "both" else n_steps) and stats[i]["accepted"] > 0
        a, b = state_of(caches[i], form), state_of(owns[i], form)
        assert (a[0] is None or np.array_equal(a[0], b[0])) and a[1:] == b[1:], (name, form)
        assert (lps[i] is None) == (i % 2 == 0) and (lps[i] is None or len(lps[i][0]) == len(want))


def test_refusals_modify_nothing(fa):
    gm = model(fa, "llama_a", "f32")
    mem = pack(fa, "llama_a", "f32")
    caches = [m[0] for m in mem]
    before = [state_of(c, f) for c, f in zip(caches, PACK_FORMS)]
    V = synth.CONFIGS["llama_a"]["vocab_size"]
    calls = [
        lambda: gm.verify_packed_lp(caches, [m[2] for m in mem], [np.zeros(17, np.uint32)] * 4, [L] * 4),          # too many drafts
        lambda: gm.verify_packed_lp(caches, [V] * 4, [m[3] for m in mem], [L] * 4),                                 # an id outside the vocabulary
        lambda: gm.verify_packed_lp(caches, [m[2] for m in mem], [m[3] for m in mem], [L] * 4, logprobs=[21] * 4),  # top_n above FL_LOGPROBS_MAX_TOP
        lambda: gm.verify_packed_lp(caches[:1] * 2, [1, 1], [[], []], [L] * 2),                                     # the same cache twice
    ]
    for call in calls:
        with pytest.raises(fa.FastLLMError) as e:
            call()
        assert e.value.code == BAD_ARGUMENT, str(e.value)
        for c, f, b in zip(caches, PACK_FORMS, before):
            a = state_of(c, f)
            assert (a[0] is None or np.array_equal(a[0], b[0])) and a[1:] == b[1:]
    # ... and n_out is zeroed: the raw call, with one member too long
    arr = (C.c_void_p * 1)(caches[0]._h)
    ids, off, pos = np.zeros(18, np.uint32), np.array([0, 18], np.uint64), np.array([L], np.uint64)
    toks, n_out = np.zeros(18, np.uint32), np.array([7], np.uint64)
    rc = fa.lib().fl_batch_verify_lp(gm._h, C.cast(arr, C.c_void_p), 1, ids.ctypes.data, off.ctypes.data, pos.ctypes.data, None, None,
                                     toks.ctypes.data, n_out.ctypes.data, None)
    assert rc == BAD_ARGUMENT and n_out[0] == 0 and len(caches[0]) == L


def test_stream_batcher_verifies_with_a_guided_slot(fa, host):  # noqa: F811
    from test_gpu_batcher_lookup import declare, sz
    from test_gpu_guide import GUIDE_ARGS, guide_args
    from test_gpu_host_mirror import BATCH_DONE_CB, BATCH_TOKEN_CB
    declare(host)
    host.flh_batcher_submit_guide_on.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, sz, sz, C.c_float, C.c_int64] + GUIDE_ARGS + \
                                                [BATCH_TOKEN_CB, BATCH_DONE_CB, C.c_void_p, C.POINTER(C.c_uint64)]
    cfg = synth.CONFIGS["llama_a"]
    gm = model(fa, "llama_a", "f32")
    base = synth.prompt_ids(cfg, 10, seed=71)
    prompts = [np.concatenate([base, base[1:], base[1:4]]).astype(np.uint32), synth.prompt_ids(cfg, 9, seed=60), synth.prompt_ids(cfg, 12, seed=64)]
    keep, gargs = guide_args(automaton_of(cfg))
    res = []
    for on in (0, 1):
        b = C.c_void_p()
        assert host.flh_batcher_create_on_lookup(gm._h, 3, 96, 4, 0, on, 7, 3, 1, 1, C.byref(b)) == 0, host.flh_last_error()
        got = {}
        cb = BATCH_TOKEN_CB(lambda rid, tok, _u: got[rid].append(int(tok)) or 1)
        dcb = BATCH_DONE_CB(lambda rid, n, _u: None)
        for i, p in enumerate(prompts):
            rid = C.c_uint64(0)
            if i == 1:                                           # the guided request, active for the whole run
                rc = host.flh_batcher_submit_guide_on(b, gm._h, p.ctypes.data, p.size, 40, 0.0, -1, *gargs, cb, dcb, None, C.byref(rid))
            else:
                rc = host.flh_batcher_submit(b, p.ctypes.data, p.size, 32, 0.0, -1, cb, dcb, None, C.byref(rid))
            assert rc == 0, host.flh_last_error()
            got[rid.value] = []
        steps, pre, v, d, a = sz(0), sz(0), sz(0), sz(0), sz(0)
        assert host.flh_batcher_run(b, C.byref(steps), C.byref(pre)) == 0, host.flh_last_error()
        assert host.flh_batcher_lookup_stats(b, C.byref(v), C.byref(d), C.byref(a)) == 0
        host.flh_batcher_destroy(b)
        res.append((got, v.value, a.value))
    (off_ids, off_v, _), (on_ids, on_v, on_a) = res
    assert off_v == 0 and on_v > 0 and on_a > 0
    assert on_ids == off_ids and [len(x) for x in on_ids.values()] == [32, 40, 32]
