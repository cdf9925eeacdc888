"""The selection kernel of a sampled verify step alone (fl_op_verify_sample, verify_sample_kernel).

Row i of a call is drawn with word draws_done + i of the seeded stream by the code select_advance runs for one row, so
  1. tokens[i] == op_sample(row i, 1, .., draws_done = w0 + i)[0] EXACTLY, and kept[i] is that call's kept count;
  2. against topp_checker.Checker driven by the oracle's ChaCha12 stream the bar of test_gpu_top_p.py holds: a differing draw sits
     within tc.MARGIN of a boundary, at most one per parametrised case;
  3. n_accepted is the numpy scan of the draft against the returned tokens, for the five drafts of test_gpu_verify_select.py;
  4. giving the rows in another order changes each position's token only through its row (row and scratch strides).
Word offsets: 0; 10 (T = 16 crosses a ChaCha block); 2^32 - 3 (the carry into the high word happens inside the call)."""
import numpy as np
import pytest

import topp_checker as tc
from oracle import oracle
from test_gpu_top_p import hard_logits

pytestmark = pytest.mark.gpu

VS = [1, 63, 1025, 4097, 32000, 152064]                 # 4097: one key past a top_filter band
TS = [1, 2, 16]
SAMPLERS = [dict(temperature=1.0), dict(temperature=0.7, top_p=0.9), dict(temperature=1.3, top_k=40),
            dict(temperature=0.8, top_p=0.9, top_k=5)]
OFFSETS = [0, 10, 2 ** 32 - 3]
SEED = 5


@pytest.fixture(scope="module")
def fa():
    import fastllm_amd
    assert fastllm_amd.device_count() >= 1
    return fastllm_amd


def word(seed, index):
    """word `index` of the oracle's seeded ChaCha12 stream"""
    o = oracle.Sampler(seed, 1.0)
    o._s.rng.word = index
    return o.next_u32()


def scan(draft, toks):
    n = 0
    while n < len(draft) and int(draft[n]) == int(toks[n]):
        n += 1
    return n


def drafts(toks, V):
    """all right, wrong at 0, wrong at the last position, right after a wrong one, all wrong (test_gpu_verify_select.py's five)"""
    right = np.array(toks[:-1], np.uint32)
    out = [right.copy()]
    if right.size:
        for at in ([0], [right.size - 1], [min(1, right.size - 1)], list(range(right.size))):
            d = right.copy()
            d[at] = (d[at] + 1) % max(V, 2)              # (V = 1: id 1 is outside the vocabulary, which a draft may be)
            out.append(d)
    return out


_rows = {}


def rows_of(V):
    if V not in _rows:
        _rows[V] = (np.random.RandomState(V + 1).randn(16, V) * 2.5).astype(np.float32)
    return _rows[V]


def one_row_reference(fa, lg, sp, w0):
    """what the one-row selection launch gives for every row with its word"""
    toks, kept = [], []
    for i, row in enumerate(lg):
        t, k = fa.op_sample(row, 1, sp["temperature"], SEED, draws_done=w0 + i, top_p=sp.get("top_p"), top_k=sp.get("top_k"), return_kept=True)
        toks.append(int(t[0]))
        kept.append(int(k[0]))
    return toks, kept


@pytest.mark.parametrize("sp", SAMPLERS, ids=lambda s: "t%g_p%s_k%s" % (s["temperature"], s.get("top_p"), s.get("top_k")))
@pytest.mark.parametrize("V", VS)
def test_rows_equal_one_row_draws(fa, V, sp):
    lg = rows_of(V)
    chks = [tc.Checker(tc.prs_of(r, sp["temperature"]), sp.get("top_p"), sp.get("top_k")) for r in lg]
    if "top_p" in sp:
        # no row may sit at the cut: a 1-ulp difference in an exp would then move m, and the test would be about expf (test_gpu_top_p.py)
        assert min(c.margin for c in chks) > 4 * float(np.spacing(np.float32(sp["top_p"]))), "a row within 4 ulp of the cut"
    n_diff = 0
    for w0 in OFFSETS:
        want, want_kept = one_row_reference(fa, lg, sp, w0)
        for i, chk in enumerate(chks):                   # the one-row draws themselves, against the checker
            tok, near = chk.draw(word(SEED, w0 + i))
            assert want_kept[i] == chk.m, (V, sp, i, want_kept[i], chk.m)
            if tok != want[i]:
                n_diff += 1
                assert near <= tc.MARGIN, "V %d row %d word %d: device %d checker %d, %.3g from a boundary" % (V, i, w0 + i, want[i], tok, near)
        for T in TS:
            for d in drafts(want[:T], V):
                toks, n_acc, kept = fa.op_verify_sample(lg[:T], d, sp["temperature"], seed=SEED, draws_done=w0, top_p=sp.get("top_p"),
                                                        top_k=sp.get("top_k"), return_kept=True)
                assert toks.tolist() == want[:T], (V, sp, w0, T)
                assert kept.tolist() == want_kept[:T], (V, sp, w0, T)
                assert n_acc == scan(d, toks), (V, sp, w0, T, d.tolist(), toks.tolist())
    assert n_diff <= 1, n_diff


@pytest.mark.parametrize("shape,top_p", [("flat", 0.9), ("one_hot", 0.9), ("tiny_tail", 0.5), ("ties", 0.9)])
def test_hard_inputs_at_16_rows(fa, shape, top_p):
    row = hard_logits(shape)
    lg = np.tile(row, (16, 1))
    for w0 in (0, 10):
        want, want_kept = fa.op_sample(row, 16, 1.0, 1, draws_done=w0, top_p=top_p, return_kept=True)
        toks, n_acc, kept = fa.op_verify_sample(lg, want[:15], 1.0, seed=1, draws_done=w0, top_p=top_p, return_kept=True)
        assert np.array_equal(toks, want) and np.array_equal(kept, want_kept) and n_acc == 15
        chk = tc.Checker(tc.prs_of(row, 1.0), top_p)
        assert (kept == chk.m).all()
        assert tc.compare_draws(toks, chk, 1, draws_done=w0) <= 1


def test_rows_in_another_order(fa):
    V = 4097
    lg = rows_of(V)
    sp = SAMPLERS[1]
    perm = np.random.RandomState(3).permutation(16)
    assert (perm != np.arange(16)).any()
    for w0 in (0, 2 ** 32 - 3):
        toks, _ = fa.op_verify_sample(lg[perm], np.zeros(15, np.uint32), sp["temperature"], seed=SEED, draws_done=w0, top_p=sp["top_p"])
        for pos, r in enumerate(perm):
            one = fa.op_sample(lg[r], 1, sp["temperature"], SEED, draws_done=w0 + pos, top_p=sp["top_p"])
            assert toks[pos] == one[0], (pos, r)
    # (the rows do differ: the same word on two rows gives two tokens somewhere)
    a = [int(fa.op_sample(lg[r], 1, sp["temperature"], SEED, draws_done=0, top_p=sp["top_p"])[0]) for r in range(16)]
    assert len(set(a)) > 4
