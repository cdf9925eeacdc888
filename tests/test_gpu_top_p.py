"""Nucleus (top-p) and top-k sampling in the device token selection (fl_*_sample_ex) against the numpy restatement of candle's
Sampling::TopP / TopK / TopKThenTopP in topp_checker.py.  The bar is that of test_gpu_sampler.py: the same token on every draw (at
most 1 in 400 may differ, and only where `chosen` is within 1e-6 of a boundary), and the kept count equals the checker's m exactly.
"""
import numpy as np
import pytest

import synth
import topp_checker as tc
from oracle import oracle

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fa():
    import fastllm_amd
    assert fastllm_amd.device_count() >= 1
    return fastllm_amd


def check(fa, lg, n, temperature, seed, top_p=None, top_k=None):
    got, kept = fa.op_sample(lg, n, temperature, seed, top_p=top_p, top_k=top_k, return_kept=True)
    chk = tc.Checker(tc.prs_of(lg, temperature), top_p, top_k)
    print("V %d T %g top_p %s top_k %s: m %d kept %s margin %s" % (lg.size, temperature, top_p, top_k, chk.m, sorted(set(kept.tolist())), chk.margin))
    assert got.max() < lg.size
    n_diff = tc.compare_draws(got, chk, seed)
    assert n_diff <= 1, n_diff
    assert (kept == chk.m).all(), (sorted(set(kept.tolist())), chk.m)
    return got, chk


@pytest.mark.parametrize("V,temperature,top_p,seed,m", [(320, 0.8, 0.9, 0, 25), (32000, 1.0, 0.9, 0, 3662), (32000, 0.3, 0.5, 11, 1),
                                                        (152064, 0.7, 0.95, 0, 3712), (151, 1.5, 0.8, 3, 22),
                                                        (50257, 2.0, 0.99, 123456789, 43175)])
def test_top_p_draws_match_checker(fa, V, temperature, top_p, seed, m, monkeypatch):
    lg = (np.random.RandomState(V + seed).randn(V) * 2.5).astype(np.float32)
    chk = tc.Checker(tc.prs_of(lg, temperature), top_p)
    # the input must not sit at the cut: a 1-ulp difference in an exp would then move m, and the test would be about expf
    assert chk.margin > 4 * float(np.spacing(np.float32(top_p))), "input within 4 ulp of the cut: %.3g" % chk.margin
    assert chk.m == m, (chk.m, m)
    got, _ = check(fa, lg, 400, temperature, seed, top_p=top_p)
    # the one-lane walk of the two sums gives the same tokens
    monkeypatch.setenv("FL_SAMPLE_WALK", "1")
    np.testing.assert_array_equal(fa.op_sample(lg, 400, temperature, seed, top_p=top_p), got)


def hard_logits(shape):
    V = 32768
    rs = np.random.RandomState(7)
    if shape == "flat":
        return np.zeros(V, np.float32)
    if shape == "one_hot":
        lg = np.full(V, -200.0, np.float32); lg[777] = 0.0
        return lg
    if shape == "tiny_tail":
        return np.concatenate([np.full(64, 5.0), np.full(V - 64, -12.0)]).astype(np.float32)
    return (np.log(2.0) * rs.randint(-20, 1, size=V)).astype(np.float32)         # ties: powers of two


@pytest.mark.parametrize("shape,top_p,m", [("flat", 0.9, 29492), ("tiny_tail", 0.5, 32), ("tiny_tail", 0.9999, 64), ("one_hot", 0.9, 1),
                                           ("ties", 0.9, None)])
def test_top_p_hard_inputs(fa, shape, top_p, m):
    lg = hard_logits(shape)
    got, chk = check(fa, lg, 300, 1.0, 1, top_p=top_p)
    if m is not None:
        assert chk.m == m, (chk.m, m)
    if shape == "tiny_tail" and top_p == 0.5:
        assert got.max() < 32
    if shape == "one_hot":
        assert (got == 777).all()
    if shape == "ties":
        # the cut falls inside a run of equal probabilities: the lower indices of the run are the kept ones
        prs = tc.prs_of(lg, 1.0)
        last = chk.order[chk.m - 1]
        run = np.flatnonzero(prs == prs[last])
        assert run.size > 1 and run[0] <= last < run[-1], "the cut does not split a run of ties"
        dropped = set(run[run > last].tolist())
        assert not dropped & set(got.tolist())


def test_identities(fa):
    V = 1000
    lg = (np.random.RandomState(1).randn(V) * 3).astype(np.float32)
    base = fa.op_sample(lg, 50, 0.9, 4)
    for p in (0.0, 1.0, 1.5):
        got, kept = fa.op_sample(lg, 50, 0.9, 4, top_p=p, return_kept=True)
        np.testing.assert_array_equal(got, base)
        assert (kept == V).all()
    for k in (0, V, V + 1):
        got, kept = fa.op_sample(lg, 50, 0.9, 4, top_k=k, return_kept=True)
        np.testing.assert_array_equal(got, base)
        assert (kept == V).all()
    # draws_done positions the stream as it does without a filter (on flatter logits, whose nucleus holds hundreds of tokens -- `lg`
    # keeps 3 -- so that a stream stuck at one word would show)
    lg2 = np.random.RandomState(2).randn(V).astype(np.float32)
    assert tc.kept_prefix(tc.prs_of(lg2, 0.9), top_p=0.9)[1] > 100
    a = fa.op_sample(lg2, 25, 0.9, 4, top_p=0.9)
    b = fa.op_sample(lg2, 20, 0.9, 4, draws_done=5, top_p=0.9)
    np.testing.assert_array_equal(a[5:], b)
    assert len(set(a.tolist())) > 5
    # top_k = 40 with top_p = 0.9 keeps min(40, m)
    _, m, _ = tc.kept_prefix(tc.prs_of(lg, 0.9), top_p=0.9)
    _, chk = check(fa, lg, 100, 0.9, 4, top_p=0.9, top_k=40)
    assert chk.m == min(40, m)
    _, chk = check(fa, lg, 100, 0.9, 4, top_p=0.999, top_k=40)
    assert chk.m == 40


def test_top_k_one_is_the_first_maximal_index_and_argmax_the_last(fa):
    lg = np.zeros(5000, dtype=np.float32)
    lg[[17, 4321]] = 3.0
    got, kept = fa.op_sample(lg, 5, 1.0, 0, top_k=1, return_kept=True)
    assert got.tolist() == [17] * 5 and kept.tolist() == [1] * 5
    # temperature < 1e-7 stays ArgMax whatever the other fields say
    got, kept = fa.op_sample(lg, 3, 0.0, 0, top_p=0.5, top_k=1, return_kept=True)
    assert got.tolist() == [4321] * 3 and kept.tolist() == [5000] * 3


def test_top_k_distribution(fa):
    rs = np.random.RandomState(5)
    lg = (rs.randn(64) * 1.5).astype(np.float32)
    n = 50000
    got = fa.op_sample(lg, n, 0.9, 2, top_k=8)
    p = np.exp(lg.astype(np.float64) / 0.9)
    top = np.argsort(-p, kind="stable")[:8]
    q = p[top] / p[top].sum()
    counts = np.bincount(got, minlength=64)
    assert counts.sum() == counts[top].sum(), "a token outside the top 8 was drawn"
    chi2 = ((counts[top] - n * q) ** 2 / (n * q)).sum()
    print("chi2 %.3f" % chi2)
    assert chi2 < 24.3, chi2                          # 7 dof: 99.9th percentile


def teacher_forced(gm, ids, toks, temp, top_p=None, top_k=None):
    """the device's own logits along its own token sequence, sampled by the checker"""
    T = len(ids)
    c2 = gm.new_cache(64)
    o = oracle.Sampler(0, 1.0)
    lg = gm.forward(c2, ids, 0)
    for i in range(len(toks)):
        tok, near = tc.Checker(tc.prs_of(lg, temp), top_p, top_k).draw(o.next_u32())
        if tok != toks[i]:
            assert near <= tc.MARGIN, "step %d: device %d checker %d" % (i, toks[i], tok)
        if i + 1 < len(toks):
            lg = gm.forward(c2, [toks[i]], T + i)


@pytest.mark.parametrize("name,dtype", [("llama_a", "f32"), ("qwen2_a", "bf16")])
def test_generate_with_top_p(fa, name, dtype):
    cfg = synth.CONFIGS[name]
    gm = fa.Model(cfg, synth.synth_weights(cfg), dtype=dtype)
    ids = synth.prompt_ids(cfg, 9, seed=2)
    T, n, temp = len(ids), 24, 0.8

    def single(top_p=None, top_k=None, t=temp):
        c = gm.new_cache(64)
        if t is None:
            first = gm.forward_argmax(c, ids, 0)
            return c, [first] + gm.decode_greedy(c, first, T, n - 1).tolist()
        first = gm.forward_sample(c, ids, 0, t, top_p=top_p, top_k=top_k)
        return c, [first] + gm.decode_sample(c, first, T, n - 1, t, draws_done=1, top_p=top_p, top_k=top_k).tolist()

    gc, toks = single(top_p=0.9)
    assert len(toks) == n and len(gc) == T + n - 1
    teacher_forced(gm, ids, toks, temp, top_p=0.9)
    _, toks_pk = single(top_p=0.9, top_k=5)
    teacher_forced(gm, ids, toks_pk, temp, top_p=0.9, top_k=5)
    # one batch mixing ArgMax, Sampling::All and top-p + top-k: every stream equals its single-stream run
    _, toks_greedy = single(t=None)
    _, toks_all = single()
    caches = [gm.new_cache(64) for _ in range(3)]
    firsts = [gm.forward_argmax(caches[0], ids, 0), gm.forward_sample(caches[1], ids, 0, temp),
              gm.forward_sample(caches[2], ids, 0, temp, top_p=0.9, top_k=5)]
    rows = fa.Batch(gm, caches).decode_each(firsts, [T] * 3, n - 1, temperatures=[None, temp, temp], top_p=[None, None, 0.9],
                                            top_k=[None, None, 5])
    for first, row, want in zip(firsts, rows, (toks_greedy, toks_all, toks_pk)):
        assert [first] + row.tolist() == want
    # a greedy call afterwards is ArgMax again (the selection state belongs to the call, not the cache)
    c3 = gm.new_cache(64)
    assert gm.forward_argmax(c3, ids, 0) == oracle.argmax(gm.forward(gm.new_cache(64), ids, 0))
