"""The logit-rules kernel alone (fl_op_logit_rules, the batch form) against the numpy float32 restatement of
tests/logit_rules_ref.py: adjusted rows AND table words bit for bit.

Shapes: V = 5 (one scalar chunk and a tail), 320 (the test models' vocabulary), 1003 (odd: rows b > 0 start off a 16-byte boundary, so
they take the scalar path while row 0 takes the vector path and a 3-id tail) and 32 000 (32 workgroups per row), each as one row and
as three.  The counted token sits at id 0, at id V - 1, or nowhere; in the three-row case one row has a null table entry and must be
copied through."""
import numpy as np
import pytest

import logit_rules_ref as lr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fa():
    import fastllm_amd
    assert fastllm_amd.device_count() >= 1
    return fastllm_amd


def case(B, V, seed):
    """Rows with every kind of entry: unseen ids, prompt-only ids, counted ids with and without the prompt bit, finite and -inf
    biases, and logits that are zero, negative, -inf and exactly tied."""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((B, V)) * 4).astype(np.float32)
    words = np.zeros((B, V), np.uint32)
    kind = rng.integers(0, 4, (B, V))
    words[kind == 1] = lr.PROMPT_BIT
    counts = rng.integers(1, 40, (B, V)).astype(np.uint32)
    words[kind == 2] = counts[kind == 2]
    words[kind == 3] = counts[kind == 3] | lr.PROMPT_BIT
    bias = np.where(rng.random((B, V)) < 0.1, rng.standard_normal((B, V)) * 3, 0).astype(np.float32)
    for b in range(B):
        x[b, rng.integers(0, V)] = 0.0
        x[b, rng.integers(0, V)] = -np.inf
        bias[b, rng.integers(0, V)] = -np.inf
        x[b, V - 1] = x[b, 0]                                           # an exact tie across the row
    scalars = np.asarray([[1.3, 0.5, 0.25], [0.8, -0.5, 0.0], [1.0, 0.0, 1.5]], np.float32)[:B]
    return x, words, bias, scalars


@pytest.mark.parametrize("where", ["first", "last", "absent"])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("V", [5, 320, 1003, 32000])
def test_kernel_matches_the_restatement(fa, V, B, where):
    x, words, bias, scalars = case(B, V, 1000 * B + V)
    token = {"first": 0, "last": V - 1, "absent": 0xFFFFFFFF}[where]
    tokens = np.full(B, token, np.uint32)
    has = np.ones(B, np.uint8)
    if B == 3:
        has[1] = 0                                                      # a batch member without rules
        tokens[2] = V // 2                                              # ... and one whose token sits in the middle
    got, words_after = fa.op_logit_rules(x, words, bias, scalars, tokens, count_input=True, has_rules=has)
    for b in range(B):
        if not has[b]:
            assert np.array_equal(lr.bits(got[b]), lr.bits(x[b])) and np.array_equal(words_after[b], words[b]), (V, b)
            continue
        w = lr.count(words[b].copy(), tokens[b])
        want = lr.apply(x[b], w, bias[b], *scalars[b])
        assert np.array_equal(words_after[b], w), (V, b)
        bad = np.flatnonzero(lr.bits(got[b]) != lr.bits(want))
        assert bad.size == 0, (V, b, bad[:8], got[b][bad[:8]], want[bad[:8]])


def test_a_full_count_saturates(fa):
    """2^31 - 1 outputs of one id: one more leaves the word as it is (never a carry into the prompt bit); (float)c is 2^31."""
    x = np.asarray([[1.0, 2.0, 3.0, -1.0, 0.5]], np.float32)
    words = np.asarray([[0, 0, 0x7FFFFFFF, 0xFFFFFFFF, 1]], np.uint32)
    bias = np.zeros((1, 5), np.float32)
    scalars = np.asarray([[1.0, 1e-9, 0.0]], np.float32)
    for token in (2, 3):
        got, after = fa.op_logit_rules(x, words, bias, scalars, [token])
        assert np.array_equal(after, words)
        assert np.array_equal(lr.bits(got[0]), lr.bits(lr.apply(x[0], words[0], bias[0], *scalars[0])))


def test_count_input_off_counts_nothing(fa):
    x, words, bias, scalars = case(3, 1003, 7)
    tokens = np.asarray([0, 500, 1002], np.uint32)
    got, words_after = fa.op_logit_rules(x, words, bias, scalars, tokens, count_input=False)
    assert np.array_equal(words_after, words)
    for b in range(3):
        assert np.array_equal(lr.bits(got[b]), lr.bits(lr.apply(x[b], words[b], bias[b], *scalars[b]))), b
