"""The selection kernel of a packed verify step alone (fl_op_verify_packed, verify_packed_kernel), on random logits.

A pack is the rows of several members back to back; row i of member s is selected as the member's sampler says, so
  1. an ArgMax row's id is numpy's argmax_last of the row (planted exact ties: the LAST index wins), its kept count V;
  2. a sampled row's id and kept count are EXACTLY what the one-row selection launch (op_sample) gives for that row with word
     draws_done_s + i -- also where the member starts at word 2^32 - 3 and the carry into the high word happens inside it;
  3. n_acc[s] is the numpy scan of the member's draft against the returned ids, for drafts that are right, wrong at 0 and wrong in
     the middle (the variant rotates over the members, so one launch finishes members of every kind);
  4. cutting the rows into launches of 5 or 16 rows (members straddle launches, several members finish in one launch) changes nothing;
  5. calling the op twice from Python gives the same result: the ticket words were put back (the op itself runs everything twice on the
     same buffers and fails loudly if the two passes differ).
In the MIXED 64 x 16 = 1024-row pack three members sample (the first, one in the middle, the last) and 61 are ArgMax; the sampled
one has all 64 sampling.  One-row reference draws are computed once per (row, sampler, word) and shared by every launch geometry."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

VS = [200, 1003, 32000]                                   # 1003: not a multiple of 4 (the scalar tail of argmax_last, unaligned rows)
PACKS = {"one_row": [1], "one_of_16": [16], "ragged": [1, 8, 16, 3], "full": [16] * 64}
BLOCKS = [0, 5, 16]
# per member, cycled: ArgMax | temperature 0.8 top-p 0.9 seed 3 | temperature 1.0 top-k 5 | plain temperature sampling
KINDS = [None, dict(temperature=0.8, top_p=0.9, seed=3), dict(temperature=1.0, top_k=5, seed=4), dict(temperature=1.3, seed=5)]
CARRY = 2 ** 32 - 3


@pytest.fixture(scope="module")
def fa():
    import fastllm_amd
    assert fastllm_amd.device_count() >= 1
    return fastllm_amd


def argmax_last(row):
    return int(row.size - 1 - np.argmax(row[::-1]))


def scan(draft, toks):
    n = 0
    while n < len(draft) and int(draft[n]) == int(toks[n]):
        n += 1
    return n


_logits = {}


def logits_of(V, T):
    """[T][V] random rows (the same first rows for every T of a V), every third row with a planted exact tie at its maximum"""
    key = (V, T)
    if key not in _logits:
        lg = (np.random.RandomState(V + 7).randn(T, V) * 2.5).astype(np.float32)          # (row-major fill: the same first rows for every T)
        for r in range(0, T, 3):
            a, b = sorted(np.random.RandomState(r).choice(V, 2, replace=False))
            lg[r, a] = lg[r, b] = lg[r].max() + np.float32(1.0)
        _logits[key] = lg
    return _logits[key]


def member_kinds(counts, mode):
    """per member: None (ArgMax) or a sampler dict with its own draws_done"""
    out = []
    for s in range(len(counts)):
        if mode == "argmax":
            k = None
        elif mode == "sampled":
            k = KINDS[1 + s % 3]
        elif len(counts) == 64:
            k = KINDS[1 + s % 3] if s in (0, 31, 63) else None            # (the 1024-row pack: see the module docstring)
        else:
            k = KINDS[(s + 1) % 4]                                        # mixed: members 0, 1, 2 sample, member 3 is ArgMax, ...
        if k is not None:
            k = dict(k, draws_done=CARRY if s % 2 == 0 else 10 + s)       # 10 + 16 rows crosses a ChaCha block; CARRY + 16 the 32-bit word
        out.append(k)
    return out


_ref = {}


def expected_rows(fa, V, lg, counts, kinds):
    """(ids, kept) every row must come out with: numpy for ArgMax rows, the one-row selection launch for sampled rows"""
    ids, kept, r = [], [], 0
    for cnt, k in zip(counts, kinds):
        for i in range(cnt):
            if k is None:
                ids.append(argmax_last(lg[r]))
                kept.append(V)
            else:
                key = (V, r, k["temperature"], k.get("top_p"), k.get("top_k"), k["seed"], k["draws_done"] + i)
                if key not in _ref:
                    t, kp = fa.op_sample(lg[r], 1, k["temperature"], k["seed"], draws_done=k["draws_done"] + i, top_p=k.get("top_p"),
                                         top_k=k.get("top_k"), return_kept=True)
                    _ref[key] = (int(t[0]), int(kp[0]))
                ids.append(_ref[key][0])
                kept.append(_ref[key][1])
            r += 1
    return ids, kept


def members_with_drafts(want, counts, V, shift):
    """member s's ids [token, *draft]: the draft is what the rows will give (right), wrong at 0, or wrong in the middle, by (s + shift) % 3"""
    out, r = [], 0
    for s, cnt in enumerate(counts):
        d = np.array(want[r: r + cnt - 1], np.uint32)
        variant = (s + shift) % 3
        if d.size and variant == 1:
            d[0] = (d[0] + 1) % V
        if d.size and variant == 2:
            d[d.size // 2] = (d[d.size // 2] + 1) % V
        out.append(np.concatenate([[s % V], d]).astype(np.uint32))
        r += cnt
    return out


def lists(kinds, field, default=None):
    return [default if k is None else k.get(field, default) for k in kinds]


@pytest.mark.parametrize("mode", ["argmax", "sampled", "mixed"])
@pytest.mark.parametrize("pack", list(PACKS))
@pytest.mark.parametrize("V", VS)
def test_pack(fa, V, pack, mode):
    counts = PACKS[pack]
    T = sum(counts)
    lg = logits_of(V, T)
    kinds = member_kinds(counts, mode)
    want, want_kept = expected_rows(fa, V, lg, counts, kinds)
    tied = [r for r in range(0, T, 3)]
    assert all((lg[r] == lg[r].max()).sum() == 2 for r in tied)                    # the planted ties are there, bit for bit
    kw = {}
    if mode != "argmax":
        kw = dict(temperatures=lists(kinds, "temperature"), seeds=lists(kinds, "seed"), top_p=lists(kinds, "top_p"), top_k=lists(kinds, "top_k"),
                  draws_done=lists(kinds, "draws_done"))
    starts = np.concatenate([[0], np.cumsum(counts)])
    for shift in ((0, 1, 2) if pack != "full" else (1,)):
        members = members_with_drafts(want, counts, V, shift)
        want_acc = [scan(m[1:], want[starts[s]: starts[s + 1]]) for s, m in enumerate(members)]
        if len(counts) >= 3 and counts[1] > 2:
            assert len(set(want_acc[:3])) > 1                                      # (the variants do give different counts)
        for block in BLOCKS:
            res = [fa.op_verify_packed(lg, members, block_rows=block, return_kept=True, **kw) for _ in range(2)]
            toks, acc, kept = res[0]
            assert toks.tolist() == want, (V, pack, mode, shift, block)
            assert kept.tolist() == want_kept, (V, pack, mode, shift, block)
            assert acc.tolist() == want_acc, (V, pack, mode, shift, block, acc.tolist(), want_acc)
            for x, y in zip(res[0], res[1]):                                       # the second call met tickets that were put back
                assert np.array_equal(x, y)


def test_nan_rows_select_as_the_one_row_argmax(fa):
    """NaN is handled as in select_advance: a row with NaNs gives what op_verify_select gives for it"""
    V = 1003
    lg = logits_of(V, 4).copy()
    lg[1, 17] = np.nan
    lg[2, :] = np.nan
    members = [np.zeros(3, np.uint32), np.zeros(1, np.uint32)]
    toks, acc = fa.op_verify_packed(lg, members)
    one, _ = fa.op_verify_select(lg, np.zeros(3, np.uint32))
    assert toks.tolist() == one.tolist()


def test_timed_form_returns_a_time(fa):
    lg = logits_of(200, 28)
    out = fa.op_verify_packed(lg, members_with_drafts([0] * 28, [1, 8, 16, 3], 200, 0), iters=3)
    assert len(out) == 3 and out[2] > 0.0
