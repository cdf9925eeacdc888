"""verify_adjust_packed_kernel and rules_count_packed_kernel alone (fl_op_verify_adjust_packed), bit for bit against
tests/verify_adjust_ref.py applied per member.

One pack per case: members of 1, 2, 16 and 7 rows; V 7: below one vector, odd; 513: odd, rows > 0 unaligned; 1030: V % 4 = 2, a second
chunk of 6 ids; 2051: three chunks.  block_rows = 5: the 16-row member straddles four launches; it repeats an id, has ids in different
chunks and one at the saturating count.  Guide state 0 allows all V ids, state 1 ids below 3 only, state 2 a spread with the last id."""
import numpy as np
import pytest

import fastllm_amd as fa
import guide_ref
import logit_rules_ref as lr
import verify_adjust_ref as va

pytestmark = pytest.mark.gpu

COUNTS = [1, 2, 16, 7]
KINDS = {"rules": ["r", "", "r", "r"], "guide": ["g", "", "g", "g"], "both": ["g", "", "rg", "r"]}


def make_pack(V, seed):
    rng = np.random.default_rng(seed)
    off = np.concatenate([[0], np.cumsum(COUNTS)])
    T = int(off[-1])
    x = (rng.standard_normal((T, V)) * 3).astype(np.float32)
    ids = rng.integers(0, V, T).astype(np.uint32)
    big = ids[off[2]:off[3]]                                   # the 16-row member
    big[0], big[1], big[2] = 1 % V, V - 1, V // 2              # first chunk, the last id (the scalar tail), the middle
    big[3] = big[9] = (V // 2 + 1) % V                         # twice: rows 3..8 see one count, rows 9.. two
    big[6] = 2 % V                                             # the saturated word
    words = np.zeros((4, V), np.uint32)
    bias = np.zeros((4, V), np.float32)
    for s in range(4):
        words[s], bias[s] = lr.table(V, rng.integers(0, V, 5), rng.integers(0, V, 9), {int(j): float(rng.normal()) for j in rng.integers(0, V, 4)})
        words[s][2 % V] = 0xFFFFFFFF if s == 2 else 0x7FFFFFFF
    scalars = np.array([[1.3, 0.25, 0.5], [1.0, 0.0, 0.0], [0.8, 0.125, 0.0], [1.0, 0.5, 0.75]], np.float32)
    spread = np.unique(np.concatenate([rng.integers(0, V, max(2, V // 5)), [V - 1]])).astype(np.uint32)
    au = guide_ref.Automaton([np.arange(V), np.arange(min(3, V)), spread], [1, 2, 0])
    states = rng.integers(0, 3, T).astype(np.uint32)
    states[off[2]:off[2] + 3] = [0, 1, 2]
    return off, x, ids, words, bias, scalars, au, states


@pytest.mark.parametrize("mode", ["rules", "guide", "both"])
@pytest.mark.parametrize("block_rows", [0, 5])
@pytest.mark.parametrize("V", [7, 513, 1030, 2051])
def test_packed_adjust_and_count(V, block_rows, mode):
    off, x, ids, words, bias, scalars, au, states = make_pack(V, 1000 + V)
    kinds = KINDS[mode]
    has_r = [int("r" in k) for k in kinds]
    has_g = [int("g" in k) for k in kinds]
    n_acc = np.array([0, 1, 11, 4])
    eos = np.array([-1, 3 % V, 5 % V, 6 % V])
    rng = np.random.default_rng(V)
    ret = rng.integers(0, V, ids.size).astype(np.uint32)
    for s in range(4):
        m = ret[off[s]:off[s + 1]]
        m[m == eos[s]] = (eos[s] + 1) % V
    ret[off[2] + 5] = eos[2]                                   # inside the accepted run: rows 0..5 are kept
    ret[off[3] + 6] = eos[3]                                   # behind n_acc: not a returned id, changes nothing
    keep = [1, 2, 6, 5]
    out, mid, after = fa.op_verify_adjust_packed(
        x, off, ids, words=words if mode != "guide" else None, biases=bias, scalars=scalars, has_rules=has_r,
        guide=au.csr() if mode != "rules" else None, states=states, has_guide=has_g, block_rows=block_rows, n_acc=n_acc, returned=ret, eos=eos)
    for s in range(4):
        sl = slice(int(off[s]), int(off[s + 1]))
        want = va.adjust(x[sl], ids[sl], words[s] if has_r[s] else None, bias[s], tuple(scalars[s]), au if has_g[s] else None, states[sl])
        assert np.array_equal(lr.bits(out[sl]), lr.bits(want)), (s, kinds[s])
        if not kinds[s]:
            assert np.array_equal(lr.bits(out[sl]), lr.bits(x[sl]))
    if mode == "guide":
        assert mid is None and after is None
        return
    assert np.array_equal(mid, words)                          # the adjust launches only read
    for s in range(4):
        assert np.array_equal(after[s], va.count_rows(words[s], ids[off[s]:off[s + 1]], keep[s]) if has_r[s] else words[s]), s
