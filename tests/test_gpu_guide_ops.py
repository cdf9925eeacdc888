"""guide_mask_kernel alone (fl_op_guide_mask) against the numpy restatement of tests/guide_ref.py, bit for bit: the masked rows and
the state each row was masked in.  Vocabulary sizes: 1003 (rows 1 and 2 of a [3][V] input start off a 16-byte boundary and V % 4 != 0),
4096, 32 000 and 152 064 (1 to 297 workgroups).  One automaton whose six states carry the lists a workgroup's range search can get
wrong: every id, id 0 only, id V - 1 only, the multiples of 7, every 256k - 1 and 256k (allowed ids on both sides of every
power-of-two range boundary), a seeded random half."""
import numpy as np
import pytest

import guide_ref as gr

pytestmark = pytest.mark.gpu
VOCABS = [1003, 4096, 32000, 152064]


@pytest.fixture(scope="module")
def fa():
    import fastllm_amd
    assert fastllm_amd.device_count() >= 1
    return fastllm_amd


def automaton(V):
    rng = np.random.default_rng(V)
    edge = np.arange(256, V, 256)
    lists = [np.arange(V), [0], [V - 1], np.arange(0, V, 7), np.unique(np.concatenate([edge - 1, edge])),
             np.sort(rng.choice(V, V // 2, replace=False))]
    nexts = [(np.asarray(lst, dtype=np.int64) + s + 1) % 6 for s, lst in enumerate(lists)]      # the edge depends on state and token
    return gr.Automaton(lists, nexts)


def rows(V, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((3, V)).astype(np.float32)
    x[:, 0] = -0.0                                                      # id 0 is in lists 0, 1, 3
    x[:, V - 1] = gr.NEG_INF                                            # id V - 1 is in lists 0, 2
    x[0, 7::49] = -0.0
    x[1, 255::256] = gr.NEG_INF
    x[2, 256::512] = -0.0
    x[2, 5] = gr.NEG_INF
    return x


def input_token(auto, V, state, kind):
    """kind 0: a token of the state's list; 1: one that is not (the state stays), where the list leaves one out; 2: none (>= V)."""
    lst = auto.lists[state]
    if kind == 0:
        return int(lst[len(lst) // 2])
    out = np.setdiff1d(np.arange(min(V, 64)), lst)
    return int(out[-1]) if kind == 1 and len(out) else V + 3


@pytest.mark.parametrize("V", VOCABS)
def test_masked_rows_and_states(fa, V):
    auto = automaton(V)
    x = rows(V, V + 1)
    seen = set()
    for call, entry in enumerate([(0, 1, 2), (3, 4, 5), (5, 0, 3), (2, 4, 1), (0, 4, 5), (1, 2, 3)]):
        toks = [input_token(auto, V, s, (b + call) % 3) for b, s in enumerate(entry)]
        want_state = [auto.walk(s, t) for s, t in zip(entry, toks)]
        got, states = fa.op_guide_mask(x, *auto.csr(), entry, toks)
        assert states.tolist() == want_state, (V, entry, toks)
        for b in range(3):
            want = auto.mask(x[b], want_state[b])
            assert np.array_equal(gr.bits(got[b]), gr.bits(want)), (V, entry, b, np.flatnonzero(gr.bits(got[b]) != gr.bits(want))[:8])
        seen.update(want_state)
    assert seen == set(range(6))                                        # every list masked a row


def test_rows_without_a_guide_go_through(fa):
    V = 1003
    auto = automaton(V)
    x = rows(V, 5)
    got, states = fa.op_guide_mask(x, *auto.csr(), [3, 4, 5], [V, V, V], has_guide=[1, 0, 1])
    assert states.tolist() == [3, 4, 5]
    assert np.array_equal(gr.bits(got[1]), gr.bits(x[1]))
    for b in (0, 2):
        assert np.array_equal(gr.bits(got[b]), gr.bits(auto.mask(x[b], states[b])))


def test_restatement_on_a_hand_worked_row():
    auto = gr.Automaton([[1, 3], [0]], [[1, 0], 0])
    x = np.asarray([0.5, -0.0, 2.0, gr.NEG_INF], np.float32)
    y = auto.mask(x, 0)
    assert gr.bits(y).tolist() == gr.bits(np.asarray([gr.NEG_INF, -0.0, gr.NEG_INF, gr.NEG_INF], np.float32)).tolist()
    assert auto.walk(0, 1) == 1 and auto.walk(0, 3) == 0 and auto.walk(0, 2) == 0 and auto.walk(1, 0) == 0 and auto.walk(0, 99) == 0
    assert auto.row_ptr.tolist() == [0, 2, 3] and auto.tokens.tolist() == [1, 3, 0] and auto.next.tolist() == [1, 0, 0]
    assert gr.argmax_last(np.asarray([1.0, 3.0, 3.0, gr.NEG_INF], np.float32)) == 2
