"""tests/step_ref.py has teeth on the very inputs the GPU tests use: for each of them a plausible wrong kernel gives another answer
than the reference, so an equality the GPU tests assert is not one that any implementation would meet."""
import numpy as np

import step_ref as S
from logit_rules_ref import argmax_last

VS = (151, 1003, 32000, 40000)                       # test_gpu_select_rows_ops.py's vocabularies
UNSHARD = [(tp, B, Vs) for tp in (2, 4, 8) for B in (1, 3, 8) for Vs in (4, 1000, 4004)]
SHARDS = [(k, n) for k in (1, 2, 4, 8) for n in (1, 255, 256, 257, 100003)]


def test_tie_rows_tell_first_from_last_index():
    """backs every ArgMax case of the select tests: on each tie row the first and the last maximal index differ"""
    for V in VS:
        rows = S.tie_rows(V)
        assert rows.shape[0] == 2 + sum(1 for p in S.TIE_PAIRS if p[1] < V)
        for r, row in enumerate(rows):
            assert S.argmax_first(row) != argmax_last(row), (V, r)
        assert argmax_last(rows[0]) == V - 1 and S.argmax_first(rows[0]) == 0
    assert S.tie_rows(40000).shape[0] == 7                                     # every pair of TIE_PAIRS is in play at the largest V


def test_candidate_tie_rule_and_count():
    """backs the candidate cases: the larger index wins a tie between waves, and an entry behind `count` is not read"""
    for n in (2, 64, 65, 1023):
        vals = np.zeros(n, np.float32)
        idx = np.arange(n, dtype=np.int32) * 3 + 1
        vals[[0, n - 1]] = 5.0                                                  # first and last candidate: lanes of different waves from 65 on
        assert S.cand_argmax(vals, idx) == idx[n - 1] != S.cand_argmin_index(vals, idx) == idx[0]
        vals[n - 1] = 7.0
        assert S.cand_argmax(vals, idx, n - 1) == idx[0] != S.cand_argmax(vals, idx, n)
    row = S.tie_rows(1003)[1]
    v, ix = S.chunk_candidates(row, 64)
    assert len(v) == 16 and S.cand_argmax(v, ix) == argmax_last(row) != S.cand_argmin_index(v, ix)


def test_slot_rule_depends_on_advance():
    """backs the log-prob state forms: with the start steps the GPU tests use, advance 0 and 1 put the record in the same slot only
    because the state moved -- a kernel that ignored `advance` would write one slot further"""
    for step0 in (0, 5):
        for advance in (0, 1):
            st, out, slots = S.select_run(S.state(step=step0), [7, 8, 9], advance, step0 + 3)
            assert slots == ([step0] * 3 if advance == 0 else [step0, step0 + 1, step0 + 2])
            assert S.lp_slot(st["step"], advance) != S.lp_slot(st["step"], 1 - advance)
            written = np.flatnonzero(out != S.FILL)
            assert list(written) == ([step0] if advance == 0 else [step0, step0 + 1, step0 + 2])
    assert S.lp_slot(0, 1) == 0xFFFFFFFF                                         # step < advance: past every capacity


def test_state_machine_done_is_sticky_and_eos_compares_the_token():
    st, _, _ = S.select_run(S.state(eos=4), [4, 5], 1, 2)
    assert st["done"] == 1 and st["token"] == 5 and st["step"] == 2              # set at the first launch, not cleared by the second
    st, _, _ = S.select_run(S.state(eos=-1, done=1, pos=3, len=9), [4], 1, 1)
    assert st["done"] == 1 and (st["pos"], st["len"]) == (4, 10)
    st, _, _ = S.select_run(S.state(eos=6), [4], 0, 1)
    assert st["done"] == 0 and (st["pos"], st["len"], st["step"]) == (0, 0, 0)


def test_unshard_is_neither_identity_nor_transpose():
    for tp, B, Vs in UNSHARD:
        src = np.arange(tp * B * Vs, dtype=np.float32).reshape(tp, B, Vs)
        out = S.unshard(src)
        assert out.shape == (B, tp * Vs) and sorted(out.reshape(-1)) == list(src.reshape(-1))
        if B > 1:
            assert not np.array_equal(out.reshape(-1), src.reshape(-1)), (tp, B, Vs)       # not a copy
        if B > 1 and Vs > 1:
            assert not np.array_equal(out.reshape(-1), src.transpose(1, 2, 0).reshape(-1))     # nor an element-wise transpose
        assert out[B - 1, (tp - 1) * Vs] == src[tp - 1, B - 1, 0]


def test_reduce_shards_order_shows_in_the_bits():
    """backs the reduce_shards cases: from three shards on, summing in reversed shard order changes bits of the chosen data"""
    for k, n in SHARDS:
        src = S.shard_data(k, n)
        fwd, rev = S.reduce_shards(src), S.reduce_shards(src, reverse=True)
        assert fwd.dtype == np.float32
        if k >= 3:
            assert fwd.view(np.uint32)[0] != rev.view(np.uint32)[0], (k, n)       # the planted element, so n = 1 has teeth too
            if n >= 255:
                assert (fwd.view(np.uint32)[1:] != rev.view(np.uint32)[1:]).sum() >= n // 16, (k, n)     # ... and the random ones
        else:
            assert (fwd.view(np.uint32) == rev.view(np.uint32)).all()            # one addition of two numbers commutes: no order to see


def test_gather_and_embed_formulas():
    src = np.arange(2 * 40, dtype=np.float32).reshape(2, 40)                    # 2 slabs of stride 40: 4 rows of h = 8, then 8 spare floats
    out = S.gather_last_rows(src, [3, 1], 8, 20, np.float32(-1))
    assert list(out[0, :16]) == list(range(16, 24)) + list(range(24, 32)) and (out[:, 16:] == -1).all()
    assert list(out[1, :8]) == list(range(56, 64))
    tab = np.arange(24, dtype=np.uint16).reshape(3, 8) + np.uint16(0x3F80)
    e = S.embed(tab, [2, 0, 2])
    assert e.dtype == np.float32 and (e.view(np.uint32) == (tab[[2, 0, 2]].astype(np.uint32) << 16)).all()
    assert list(S.collect([5, 6], [0, 9])) == [5, 0, 6, 9]
