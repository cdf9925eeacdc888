"""Speculative decode for full requests through the C ABI (fl_forward_verify_lp, fl_decode_lookup_lp): verify steps on caches with logit
rules, a guide, or both, with log-probs.  The cases (models, prompt seeds, rules, automaton) are test_verify_lp_margin.py's, which
asserts on the CPU that no adjusted row along their greedy continuations is a near-tie; fp32 and bf16, L = 12, n_draft in {1, 7, 15}.

  1. a step is an exact function of its own logits: from the raw rows it returns, the host restatement (verify_adjust_ref.py) gives
     the adjusted rows, ArgMax (last maximal index) or fl_op_sample_ex with word draws_done + i selects, the scan accepts -- ids and
     count equal without tolerance in both dtypes;
  2. the state after the step: the cache length, the table (the counts before + the inputs of rows 0..n_acc), the guide state;
  3. rejected rows leave no trace (the A/B construction of test_gpu_verify.py): the next 8 ruled, guided plain steps agree;
  4. log-probs: logprob_cases.check_row on the RAW row of every returned id -- the model's own distribution, not the adjusted one;
  5. the loop against the plain loop (decode_sample with log-probs) on twin caches, greedy and top-p 0.9, on a corpus that holds the
     plain continuation (accepted > 0), a random one (drafted > accepted) and, with a guide, one whose drafts are partly illegal
     (drafted below the raw draft length).  fp32: ids, table, guide state, length and number of draws equal, log-probs within
     PLAIN_LP_BOUND (derived below from the fp32 logits bar) + logprob_cases.tol of the plain loop's.  Both dtypes, every corpus and
     max_draft: the log-probs lie within logprob_cases.tol of the float64 reference of the rows the loop itself scored (stepwise()).
     bf16, ArgMax: equal to the plain loop, or at the first difference the ADJUSTED row is a near-tie
     (test_gpu_decode_lookup.same_or_near_tie's rule and number).  bf16, top-p: a deliberate deviation from "only a near-tie excuses":
     a sampled draw parts from the plain loop at a boundary of its cumulative interval, not at a top-two tie, and the loop returns no
     rows to measure that distance on; as test_gpu_verify_sample.py does, the run is bound instead by the replay -- stepwise() returns
     the same ids and log-probs one checked call at a time, and item 1 holds every such call to the sampler applied to its own rows.
     Whatever the dtype, the loop's stats are those of replaying the drafting rule on its own output;
  6. EOS inside an accepted run; 7. n_draft == 0 and max_draft == 0 are the plain _lp calls bit for bit; 8. a cache with nothing
     installed and no log-probs is forward_verify bit for bit; 9. the refusals; and the host mirror's full-request overload."""
import ctypes as C

import numpy as np
import pytest

import logit_rules_ref as lr
import logprob_cases as lc
import synth
import verify_adjust_ref as va
from test_gpu_host_mirror import generate, make  # noqa: F401
from test_gpu_parity import FP32_TOL
from test_host_mirror import host  # noqa: F401
from test_verify_lp_margin import CAP, EOS_AT, EOS_MODELS, FORMS, L, MODELS, N, SEEDS, Teacher, automaton_of, finite_scale, rules_of, top_two_gap

pytestmark = pytest.mark.gpu

GREEDY = dict(temperature=0.0, top_p=None, top_k=None, seed=0)
TOPP = dict(temperature=0.8, top_p=0.9, top_k=None, seed=7)
TOP_N = 5
# fp32 log-probs of the lookup loop against the plain loop's.  The two loops score DIFFERENT rows: a verify step's raw rows come from
# the multi-row kernels, the plain step's from the one-row kernels.  The project's fp32 bar holds every logit of either path within
# FP32_TOL of the reference (test_gpu_parity.py), so two rows x, x' of the same step differ by at most 2 FP32_TOL in every entry;
# lp_i = x_i - logsumexp(x), and logsumexp moves by at most max_j |x_j - x'_j|, so |lp_i - lp'_i| <= 2 * 2 FP32_TOL.  On top of that
# each side carries its own arithmetic, logprob_cases.tol.  (Measured on these cases: at most 6.5 tol, about 7e-5.)
PLAIN_LP_BOUND = 4 * FP32_TOL


@pytest.fixture(scope="module")
def fa():
    import fastllm_amd
    assert fastllm_amd.device_count() >= 1
    return fastllm_amd


_models, _guides, _excused = {}, {}, set()


def model(fa, name, dtype):
    if (name, dtype) not in _models:
        cfg = synth.CONFIGS[name]
        _models[(name, dtype)] = fa.Model(cfg, synth.synth_weights(cfg), dtype=dtype)
    return _models[(name, dtype)]


def guide(fa, gm, name, dtype):
    if (name, dtype) not in _guides:
        _guides[(name, dtype)] = fa.Guide(gm, *automaton_of(synth.CONFIGS[name]).csr())
    return _guides[(name, dtype)]


def start(fa, name, dtype, form, cap=CAP):
    """a cache holding the prompt, the prompt's own ArgMax, then the rules and / or the guide (state 0) installed: (cache, prompt, first)"""
    gm, cfg = model(fa, name, dtype), synth.CONFIGS[name]
    p = synth.prompt_ids(cfg, L, seed=SEEDS[name])
    c = gm.new_cache(cap)
    first = gm.forward_argmax(c, p, 0)
    if form in ("rules", "both"):
        c.set_logit_rules(**rules_of(cfg, p))
    if form in ("guide", "both"):
        c.set_guide(guide(fa, gm, name, dtype), 0)
    return c, p, first


def skw(sp, draws_done):
    return dict(temperature=sp["temperature"], top_p=sp["top_p"], top_k=sp["top_k"], seed=sp["seed"], draws_done=draws_done)


def plain_loop(fa, name, dtype, form, sp, n, eos=-1):
    """decode_sample with log-probs (fl_decode_sample_lp) on a fresh ruled, guided cache: (cache, first, tokens, token_lp, top_ids, top_lps)"""
    gm = model(fa, name, dtype)
    c, _, first = start(fa, name, dtype, form)
    toks, tlp, ids, lps = gm.decode_sample(c, first, L, n, sp["temperature"], seed=sp["seed"], draws_done=1, eos=eos, top_p=sp["top_p"],
                                           top_k=sp["top_k"], logprobs=TOP_N)
    return c, first, toks, tlp, ids, lps


def state_of(c, form):
    """(table words or None, guide state or None, cached length)"""
    return (c.logit_counts() if form in ("rules", "both") else None, c.guide_state() if form in ("guide", "both") else None, len(c))


def same_state(a, b):
    return (a[0] is None or np.array_equal(a[0], b[0])) and a[1] == b[1] and a[2] == b[2]


def selector(fa, sp, w0):
    if sp["temperature"] == 0.0:
        return lambda i, row: lr.argmax_last(row)
    return lambda i, row: int(fa.op_sample(row, 1, sp["temperature"], seed=sp["seed"], draws_done=w0 + i, top_p=sp["top_p"], top_k=sp["top_k"])[0])


def half_right(cfg, cont, n_draft):
    """test_gpu_verify.py's: the true continuation with a wrong id in the middle (n_draft >= 7)"""
    d = np.array(cont[:n_draft], np.uint32)
    if n_draft >= 7:
        d[n_draft // 2] = (d[n_draft // 2] + 1) % cfg["vocab_size"]
    return d


def check_step(fa, name, dtype, form, sp, n_draft):
    """items 1, 2 and 4 on one call; returns the accepted count"""
    gm, cfg = model(fa, name, dtype), synth.CONFIGS[name]
    case = (name, dtype, form, sp["temperature"], n_draft)
    _, first, cont, _, _, _ = plain_loop(fa, name, dtype, form, sp, 15)
    draft = half_right(cfg, cont, n_draft)
    c, p, first2 = start(fa, name, dtype, form)
    assert first2 == first
    t = Teacher(cfg, p, form)
    words0 = None if t.words is None else t.words.copy()
    toks, lg, tlp, ids, lps = gm.forward_verify_lp(c, first, draft, L, logprobs=TOP_N, want_logits=True, **skw(sp, 1))
    cut = t.cut(draft)                                                   # the rows the call forwarded: the draft the guide can reach
    inputs = [first] + cut
    rows = t.rows(lg[: len(inputs)], inputs)
    want = va.accept(rows, cut, selector(fa, sp, 1))
    assert toks.tolist() == want, (case, toks.tolist(), want)
    n_acc = len(toks) - 1
    # the state after the step
    assert len(c) == L + n_acc + 1, case
    if words0 is not None:
        assert np.array_equal(c.logit_counts(), va.count_rows(words0, inputs, n_acc + 1)), case
    if t.auto is not None:
        assert c.guide_state() == t.auto.walk_all(0, toks), case
        for i, tok in enumerate(toks):                                   # every returned id was allowed in its row's state
            assert int(tok) in t.auto.lists[t.auto.walk_all(0, inputs[1: i + 1])].tolist(), (case, i)
    # log-probs: the model's own distribution, from the raw row
    for i, tok in enumerate(toks):
        lc.check_row(lg[i], int(tok), TOP_N, tlp[i], ids[i], lps[i], what=str(case + (i,)))
    return n_acc, len(cut)


@pytest.mark.parametrize("n_draft", [1, 7, 15])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("name", MODELS)
def test_step_is_an_exact_function_of_its_own_logits(fa, name, dtype, n_draft):
    accepted = 0
    for form in FORMS:
        for sp in (GREEDY, TOPP):
            n_acc, n_cut = check_step(fa, name, dtype, form, sp, n_draft)
            accepted += n_acc
            if dtype == "f32" and sp is GREEDY and n_draft >= 7:
                assert n_acc == n_draft // 2 <= n_cut, (name, form, n_acc, n_cut)           # accepted up to the planted wrong id (which the guide may have cut)
    assert accepted > 0


@pytest.mark.parametrize("j", [0, 3, 14])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("name", ["llama_a", "mistral_a", "qwen2_a"])
def test_rejected_rows_leave_no_trace(fa, name, dtype, j):
    gm, cfg = model(fa, name, dtype), synth.CONFIGS[name]
    V, form = cfg["vocab_size"], "both"
    auto = automaton_of(cfg)
    _, first, cont, _, _, _ = plain_loop(fa, name, dtype, form, GREEDY, 15)
    right = np.array(cont, np.uint32)
    s = auto.walk_all(0, right[:j])                                      # the state row j is masked in
    legal = auto.lists[s]
    wrong = int(legal[(int(np.searchsorted(legal, right[j])) + 1) % len(legal)])          # another id that state allows: the row is forwarded, and rejected
    assert wrong != right[j]
    da = np.concatenate([right[:j], [wrong], right[j + 1:]]).astype(np.uint32)             # A: wrong at j, then more drafts
    db = right[:j]                                                       # B: the j right ones only
    outs = []
    for d in (da, db):
        c, _, _ = start(fa, name, dtype, form)
        toks, lg = gm.forward_verify_lp(c, first, d, L, want_logits=True)
        later = gm.decode_greedy(c, int(toks[-1]), L + len(toks), 8)     # 8 ruled, guided plain steps
        outs.append((toks, lg, later, state_of(c, form)))
    (ta, la, ra, sa), (tb, lb, rb, sb) = outs
    assert len(ta) <= j + 1 and np.array_equal(ta, tb), (ta, tb)
    if dtype == "f32":
        assert len(ta) == j + 1 and la.shape[0] > j + 1                  # the right drafts were accepted, and rows behind the wrong id were forwarded
    assert np.array_equal(ra, rb) and same_state(sa, sb) and sa[2] == L + len(ta) + 8


def replay(fa, t, corpus, first, got, max_draft, ngram_max, ngram_min):
    """The loop's bookkeeping replayed on its own output: (dict(steps, drafted, accepted), ids drafted before the guide cut them)."""
    hist = list(corpus) + [first]
    emitted, st, raw = 0, dict(steps=0, drafted=0, accepted=0), 0
    while emitted < len(got):
        d = fa.lookup_draft(hist, len(got) - emitted - 1, max_draft=max_draft, ngram_max=ngram_max, ngram_min=ngram_min)
        d = [int(x) for x in d]
        raw += len(d)
        dc = t.cut(d)
        n = 0
        while n < len(dc) and dc[n] == int(got[emitted + n]):
            n += 1
        ret = [int(x) for x in got[emitted: emitted + n + 1]]
        t.commit([hist[-1]] + dc[:n], ret)
        st["steps"] += 1
        st["drafted"] += len(dc)
        st["accepted"] += n
        hist += ret
        emitted += n + 1
    return st, raw


def excuse_near_tie(fa, name, dtype, form, want, k, case):
    """bf16, ArgMax: the ADJUSTED row of step k of the plain loop (one-token forwards of want[:k]) is a near-tie of its two largest
    entries -- the rule and the number of test_gpu_decode_lookup.same_or_near_tie."""
    gm, cfg = model(fa, name, dtype), synth.CONFIGS[name]
    p = synth.prompt_ids(cfg, L, seed=SEEDS[name])
    c = gm.new_cache(CAP)
    first = gm.forward_argmax(c, p, 0)
    t = Teacher(cfg, p, form)
    y = None
    for s, tok in enumerate([first] + [int(x) for x in want[:k]]):
        y = t.step_row(gm.forward(c, [tok], L + s), tok)
        t.commit([tok], [int(want[s])])
    gap, scale = top_two_gap(y), finite_scale(y)
    print("%s: differs from the plain loop at %d, adjusted top-two gap %.3e of %.3e" % (case, k, gap, scale))
    assert gap < 4e-2 * scale, "%s diverges at %d with a clear margin" % (case, k)
    _excused.add(case)
    assert len(_excused) <= 1, "more than one bf16 case needs the near-tie excuse: %s" % sorted(_excused)


def stepwise(fa, name, dtype, form, sp, corpus, first, got, got_lp, max_draft, case):
    """The loop's log-probs lie within logprob_cases.tol of the float64 log-softmax OF THE ROWS THE LOOP SCORED.  The loop returns no
    rows, so its steps are replayed one forward_verify_lp call at a time on a twin cache (the same drafts, the same launches): each
    call must return the loop's ids and -- bit for bit -- its log-probs, and logprob_cases.check_row holds them against the call's raw
    rows: a log-prob scattered to the wrong entry, or scored against the adjusted row, fails here whatever the corpus.  (tol bounds the
    arithmetic on ONE row; the distance to the plain loop's values has its own bound, PLAIN_LP_BOUND.)"""
    gm = model(fa, name, dtype)
    c, _, _ = start(fa, name, dtype, form)
    hist, emitted, tok = list(corpus) + [first], 0, first
    while emitted < len(got):
        d = fa.lookup_draft(hist, len(got) - emitted - 1, max_draft=max_draft, ngram_max=3, ngram_min=1)
        toks, lg, tlp, ids, lps = gm.forward_verify_lp(c, tok, d, L + emitted, logprobs=TOP_N, want_logits=True, **skw(sp, 1 + emitted))
        n = len(toks)
        assert np.array_equal(toks, got[emitted: emitted + n]), (case, emitted)
        sl = slice(emitted, emitted + n)
        assert np.array_equal(lr.bits(tlp), lr.bits(got_lp[0][sl])) and np.array_equal(ids, got_lp[1][sl]), (case, emitted)
        assert np.array_equal(lr.bits(lps), lr.bits(got_lp[2][sl])), (case, emitted)
        for i in range(n):
            lc.check_row(lg[i], int(toks[i]), TOP_N, got_lp[0][emitted + i], got_lp[1][emitted + i], got_lp[2][emitted + i], what="%s token %d" % (case, emitted + i))
        hist += toks.tolist()
        emitted += n
        tok = int(toks[-1])


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("name", MODELS)
def test_loop_against_the_plain_loop(fa, name, dtype):
    gm, cfg = model(fa, name, dtype), synth.CONFIGS[name]
    V = cfg["vocab_size"]
    rng = np.random.default_rng(SEEDS[name])
    worst_lp = 0.0
    for form in FORMS:
        for sp in (GREEDY, TOPP):
            twin, first, plain, ptlp, pids, plps = plain_loop(fa, name, dtype, form, sp, N)
            assert len(plain) == N
            want_state = state_of(twin, form)
            p = synth.prompt_ids(cfg, L, seed=SEEDS[name])
            clean = np.concatenate([p, [first], plain]).astype(np.uint32)
            bad = plain.copy()
            bad[4::5] = (bad[4::5] + 1) % V                              # (with a guide: j + 1 leads elsewhere than j, and is often illegal)
            corpora = dict(clean=clean, random=rng.integers(0, V, 1024).astype(np.uint32),
                           corrupted=np.concatenate([p, [first], bad]).astype(np.uint32))
            for what, corpus in corpora.items():
                for max_draft in ((7, 15) if what == "clean" else (7,)):
                    case = "%s %s %s t %g %s max_draft %d" % (name, dtype, form, sp["temperature"], what, max_draft)
                    c, _, f = start(fa, name, dtype, form)
                    got, tlp, ids, lps, st = gm.decode_lookup_lp(c, corpus, f, L, N, max_draft=max_draft, return_stats=True, logprobs=TOP_N, **skw(sp, 1))
                    assert f == first and len(got) == N and len(c) == L + N, case      # as many tokens, i.e. as many draws
                    sim, raw = replay(fa, Teacher(cfg, p, form), corpus, first, got, max_draft, 3, 1)
                    assert st == sim, (case, st, sim)
                    same = np.array_equal(got, plain)
                    if dtype == "f32":
                        assert same, (case, int(np.argmax(got != plain)))
                        assert same_state(state_of(c, form), want_state), case
                        # log-probs against the PLAIN loop's, within PLAIN_LP_BOUND + logprob_cases.tol of either side
                        assert np.array_equal(ids, pids), case
                        for a, b in ((tlp, ptlp), (lps, plps)):
                            a64, b64 = np.asarray(a, np.float64), np.asarray(b, np.float64)
                            top = np.asarray(plps[:, 0], np.float64).reshape((-1,) + (1,) * (b64.ndim - 1))
                            tol = 2.0 ** -20 * (1.0 + np.abs(b64 - top) + np.abs(b64))      # logprob_cases.tol: x_i - m = lp_i - lp_top
                            d = np.abs(a64 - b64)
                            worst_lp = max(worst_lp, float(d.max()))
                            assert (d <= PLAIN_LP_BOUND + 2 * tol).all(), (case, float(d.max()), PLAIN_LP_BOUND)
                    elif not same:
                        k = int(np.argmax(got != plain))
                        if sp is GREEDY:
                            excuse_near_tie(fa, name, dtype, form, plain, k, "bf16 " + case)
                    stepwise(fa, name, dtype, form, sp, corpus, first, got, (tlp, ids, lps), max_draft, case)      # every corpus, max_draft and dtype
                    if what == "clean" and (same or dtype == "f32"):
                        assert st["accepted"] > 0, (case, st)
                    if what == "random":
                        assert st["drafted"] > st["accepted"], (case, st)
                    if what == "corrupted" and form != "rules" and same:
                        assert st["drafted"] < raw, (case, st, raw)     # the guide cut looked-up drafts
    print("%s %s: largest log-prob difference to the plain loop %.3e (bound %.1e + tol)" % (name, dtype, worst_lp, PLAIN_LP_BOUND))


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("name", EOS_MODELS)
def test_eos_inside_an_accepted_run(fa, name, dtype):
    """The EOS is the plain loop's 16th output, so the plain loop's first chunk (16 steps) ends with the step that draws it: its table is
    then exactly "the inputs of steps 0..15" (behind an EOS inside a chunk the plain loop's table is unspecified, the header says)."""
    gm, cfg = model(fa, name, dtype), synth.CONFIGS[name]
    form, i = "both", EOS_AT
    _, first, plain, _, _, _ = plain_loop(fa, name, dtype, form, GREEDY, N)
    assert plain[i] not in plain[:i] and plain[i] != first, "the case needs an id that first comes up as output 15"
    eos = int(plain[i])
    p = synth.prompt_ids(cfg, L, seed=SEEDS[name])
    clean = np.concatenate([p, [first], plain]).astype(np.uint32)
    st, _ = replay(fa, Teacher(cfg, p, form), clean, first, plain, 7, 3, 1)
    assert st["accepted"] > 0
    twin, _, want, wtlp, _, _ = plain_loop(fa, name, dtype, form, GREEDY, N, eos=eos)
    assert np.array_equal(want, plain[:i]) and len(twin) == L + i + 1
    c, _, f = start(fa, name, dtype, form)
    got, tlp, _, _, stats = gm.decode_lookup_lp(c, clean, f, L, N, eos=eos, return_stats=True, logprobs=TOP_N)
    if dtype == "f32":
        assert np.array_equal(got, want) and stats["accepted"] > 0
    if np.array_equal(got, want):
        assert same_state(state_of(c, form), state_of(twin, form))      # tokens, length, counts and state: the plain loop's
        t = Teacher(cfg, p, form)
        t.commit([first] + plain[:i].tolist(), plain[: i + 1].tolist())
        assert np.array_equal(c.logit_counts(), t.words) and c.guide_state() == t.state
        assert len(tlp) == len(got)
        # going on from there: the twin's tokens
        assert np.array_equal(gm.decode_greedy(c, eos, L + i + 1, 6), gm.decode_greedy(twin, eos, L + i + 1, 6))
    else:
        assert len(c) == L + len(got) + (1 if len(got) < N else 0)      # the length the plain loop leaves, wherever bf16 stopped


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("name", ["llama_a", "mistral_a", "qwen2_a"])
def test_no_drafts_is_the_plain_lp_call_bit_for_bit(fa, name, dtype):
    gm, cfg = model(fa, name, dtype), synth.CONFIGS[name]
    for form in FORMS:
        for sp in (GREEDY, TOPP):
            # n_draft == 0: one step of decode_sample with log-probs
            twin, first, toks, tlp, ids, lps = plain_loop(fa, name, dtype, form, sp, 1)
            c, p, f = start(fa, name, dtype, form)
            got, lg, gtlp, gids, glps = gm.forward_verify_lp(c, f, [], L, logprobs=TOP_N, want_logits=True, **skw(sp, 1))
            assert np.array_equal(got, toks) and np.array_equal(lr.bits(gtlp), lr.bits(tlp)) and np.array_equal(gids, ids)
            assert np.array_equal(lr.bits(glps), lr.bits(lps)) and same_state(state_of(c, form), state_of(twin, form))
            raw, _, _ = start(fa, name, dtype, "none")
            assert np.array_equal(lr.bits(lg[0]), lr.bits(gm.forward(raw, [f], L)))        # logits_out is the raw row
            # a draft the guide cuts to nothing is the same step
            if form != "rules":
                t = Teacher(cfg, p, form)
                illegal = int(np.setdiff1d(np.arange(cfg["vocab_size"]), t.auto.lists[0])[0])
                c2, _, _ = start(fa, name, dtype, form)
                got2, _ = gm.forward_verify_lp(c2, f, [illegal, 1, 2], L, **skw(sp, 1))
                assert np.array_equal(got2, toks) and same_state(state_of(c2, form), state_of(twin, form))
            # max_draft == 0: the loop is decode_sample with log-probs
            twin, first, toks, tlp, ids, lps = plain_loop(fa, name, dtype, form, sp, N)
            c, p, f = start(fa, name, dtype, form)
            got, gtlp, gids, glps, st = gm.decode_lookup_lp(c, p, f, L, N, max_draft=0, return_stats=True, logprobs=TOP_N, **skw(sp, 1))
            assert np.array_equal(got, toks) and np.array_equal(lr.bits(gtlp), lr.bits(tlp)) and np.array_equal(gids, ids)
            assert np.array_equal(lr.bits(glps), lr.bits(lps)) and same_state(state_of(c, form), state_of(twin, form))
            assert st == dict(steps=N, drafted=0, accepted=0)


@pytest.mark.parametrize("n_draft", [0, 1, 7, 15])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("name", ["llama_a", "mistral_a", "qwen2_a"])
def test_a_bare_cache_is_forward_verify_bit_for_bit(fa, name, dtype, n_draft):
    gm, cfg = model(fa, name, dtype), synth.CONFIGS[name]
    for sp in (GREEDY, TOPP):
        _, first, cont, _, _, _ = plain_loop(fa, name, dtype, "none", sp, 15)
        draft = half_right(cfg, cont, n_draft)
        old = dict() if sp is GREEDY else skw(sp, 1)
        a, _, _ = start(fa, name, dtype, "none")
        b, _, _ = start(fa, name, dtype, "none")
        ta, la = gm.forward_verify(a, first, draft, L, want_logits=True, **old)
        tb, lb = gm.forward_verify_lp(b, first, draft, L, want_logits=True, **skw(sp, 1))
        assert np.array_equal(ta, tb) and np.array_equal(lr.bits(la), lr.bits(lb)) and len(a) == len(b)
        # ... and with log-probs the ids stay what they were
        d, _, _ = start(fa, name, dtype, "none")
        td, ld, tlp, ids, lps = gm.forward_verify_lp(d, first, draft, L, logprobs=TOP_N, want_logits=True, **skw(sp, 1))
        assert np.array_equal(td, ta) and np.array_equal(lr.bits(ld), lr.bits(la))
        for i, tok in enumerate(td):
            lc.check_row(ld[i], int(tok), TOP_N, tlp[i], ids[i], lps[i])
        if n_draft == 0:
            # ... and the loop on a bare cache without log-probs is decode_lookup, its draft-less steps included: the corpus holds
            # neither `first` nor the early outputs, so the first step has nothing to draft from
            early = set(cont[:8].tolist()) | {first}
            unused = [t for t in range(cfg["vocab_size"]) if t not in early and t not in cont.tolist()][:8]
            corpus = np.asarray(unused + [int(t) for t in cont[8:] if int(t) not in early], np.uint32)
            assert len(fa.lookup_draft(corpus.tolist() + [first], 14, max_draft=7, ngram_max=3, ngram_min=1)) == 0
            a, _, _ = start(fa, name, dtype, "none")
            b, _, _ = start(fa, name, dtype, "none")
            ga, sa = gm.decode_lookup(a, corpus, first, L, 15, return_stats=True, **old)
            gb, sb = gm.decode_lookup_lp(b, corpus, first, L, 15, return_stats=True, **skw(sp, 1))
            assert np.array_equal(ga, gb) and sa == sb and len(a) == len(b) == L + 15
            assert np.array_equal(lr.bits(gm.forward(a, [int(ga[-1])], L + 15)), lr.bits(gm.forward(b, [int(gb[-1])], L + 15)))


def test_refusals(fa):
    cfg = synth.CONFIGS["llama_a"]
    tp = fa.Model(cfg, synth.synth_weights(cfg), dtype="bf16", tp_mode=fa.binding.TP_EMULATED, tp_size=2)
    c = tp.new_cache(CAP)
    first = tp.forward_argmax(c, synth.prompt_ids(cfg, 5), 0)
    for call in (lambda: tp.forward_verify_lp(c, first, [1, 2], 5), lambda: tp.decode_lookup_lp(c, [1, 2, 3], first, 5, 8),
                 lambda: tp.forward_verify_lp(c, first, [1, 2], 5, logprobs=2, temperature=0.8)):
        with pytest.raises(fa.FastLLMError) as e:
            call()
        assert e.value.code == -10 and "tensor parallelism" in str(e.value) and len(c) == 5
    tp.close()
    gm = fa.Model(synth.CONFIGS["mistral_win"], synth.synth_weights(synth.CONFIGS["mistral_win"]), dtype="bf16")
    c = gm.new_cache(CAP)
    first = gm.forward_argmax(c, synth.prompt_ids(synth.CONFIGS["mistral_win"], 5), 0)
    c.set_logit_rules(frequency_penalty=0.5)
    toks, _ = gm.forward_verify_lp(c, first, [1] * 5, 5)                 # n_draft == sliding_window is served
    assert len(c) == 5 + len(toks)
    c.truncate(5)
    with pytest.raises(fa.FastLLMError) as e:
        gm.forward_verify_lp(c, first, [1] * 6, 5)
    assert e.value.code == -10 and "sliding_window" in str(e.value) and len(c) == 5
    with pytest.raises(fa.FastLLMError) as e:
        gm.forward_verify_lp(c, first, [1, 2], 5, logprobs=21)
    assert e.value.code == -8 and len(c) == 5
    with pytest.raises(fa.FastLLMError) as e:                           # the old call keeps refusing the ruled cache
        gm.forward_verify(c, first, [1, 2], 5)
    assert e.value.code == -10 and len(c) == 5
    gm.close()


@pytest.mark.parametrize("name", ["llama_a", "mistral_a", "qwen2_a"])
def test_host_mirror_full_request(host, name, monkeypatch):
    """Model<M>::generate_ids / generate_stream_ids with LookupOptions + LogitRules + GuideOptions + top_logprobs (fp32): the ids of the
    plain ruled, guided generate_ids, greedy and top-p 0.9, with one log-prob record per id."""
    monkeypatch.setenv("FASTLLM_POS_MODE", "tokens")
    monkeypatch.setenv("FASTLLM_MAX_SEQ", "96")
    vp, sz = C.c_void_p, C.c_size_t
    host.flh_generate_lookup_request.argtypes = [vp, vp, sz, sz, C.c_float, C.c_int64, C.c_double, C.c_int64, C.c_int, sz, vp, vp, C.c_float, C.c_float,
                                                 C.c_float, C.c_uint32, vp, vp, vp, C.c_uint32, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp,
                                                 C.POINTER(sz), vp, vp, vp, C.POINTER(sz), vp]
    h, cfg, _ = make(host, name, dtype=0)
    base = synth.prompt_ids(cfg, 10, seed=SEEDS[name])
    prompt = np.concatenate([base, base[1:], base[1:4]]).astype(np.uint32)       # a prompt that repeats itself: drafts from the prompt
    n = 24
    r = rules_of(cfg, prompt)
    bias_ids = np.asarray(list(r["logit_bias"]), np.uint32)
    bias_values = np.asarray(list(r["logit_bias"].values()), np.float32)
    row_ptr, tokens, nxt = automaton_of(cfg).csr()

    def request(max_draft, stream=0, top_logprobs=-1, temperature=0.0, top_p=0.0):
        out, tlp = np.zeros(n, np.uint32), np.full(n, np.nan, np.float32)
        ids, lps = np.zeros((n, TOP_N), np.uint32), np.zeros((n, TOP_N), np.float32)
        n_out, fw = sz(0), sz(0)
        st = (C.c_uint64 * 3)()
        rc = host.flh_generate_lookup_request(h, prompt.ctypes.data, prompt.size, n, temperature, -1, top_p, 0, 1, bias_ids.size, bias_ids.ctypes.data,
                                              bias_values.ctypes.data, r["repetition_penalty"], r["frequency_penalty"], r["presence_penalty"], 3,
                                              row_ptr.ctypes.data, tokens.ctypes.data, nxt.ctypes.data, 0, max_draft, 3, 1, stream, top_logprobs,
                                              out.ctypes.data, C.byref(n_out), tlp.ctypes.data, ids.ctypes.data, lps.ctypes.data, C.byref(fw), st)
        assert rc == 0, host.flh_last_error()
        return out[: n_out.value], tlp[: n_out.value], ids[: n_out.value], fw.value, list(st)

    for temperature, top_p in ((0.0, 0.0), (0.8, 0.9)):
        want, _, _, fw_plain, _ = request(-1, temperature=temperature, top_p=top_p)
        assert len(want) == n
        auto = automaton_of(cfg)
        s = 0
        for t in want:                                                   # the plain request honoured the guide
            assert int(t) in auto.lists[s].tolist()
            s = auto.walk(s, int(t))
        for stream in (0, 1):
            got, tlp, ids, fw, st = request(7, stream, TOP_N, temperature, top_p)
            np.testing.assert_array_equal(got, want)
            assert np.isfinite(tlp).all() and (tlp <= 0).all() and (ids < cfg["vocab_size"]).all()
            assert fw <= fw_plain
            if not stream:
                assert fw == 1 + st[0] and st[1] >= st[2]
            got2, _, _, _, _ = request(7, stream, -1, temperature, top_p)     # ... and without log-probs
            np.testing.assert_array_equal(got2, want)
    host.flh_model_destroy(h)
