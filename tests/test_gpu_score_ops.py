"""The scoring kernel alone (fl_op_score) against numpy float64 on the same fp32 rows: the target's log-prob and the top values within
the derived tolerance of tests/logprob_cases.py, top ids EXACTLY np.lexsort((idx, -x))[:top_n], the target's rank EXACTLY its place in
that order.  (The entry launches the kernel twice and fails if the two results differ.)"""
import numpy as np
import pytest

import score_cases as sc
from score_cases import lc
from test_gpu_logprobs_ops import NAMES

pytestmark = pytest.mark.gpu
NO = sc.NO_TARGET


@pytest.fixture(scope="module")
def fa():
    import fastllm_amd
    assert fastllm_amd.device_count() >= 1
    return fastllm_amd


@pytest.fixture(scope="module")
def rows():
    return lc.rows()


def check(fa, a, targets, top_n, what):
    a = np.ascontiguousarray(a, dtype=np.float32)
    T, V = a.shape
    res = fa.op_score(a, targets, top_n)
    assert res.target_logprob.shape == (T,) and res.target_rank.shape == (T,) and res.top_ids.shape == (T, top_n) and res.top_logprobs.shape == (T, top_n)
    assert res.logits is None and (res.top_ids < V).all()
    for t in range(T):
        sc.check_scored_row(a[t], targets[t], top_n, res, t, what=(what, top_n))
    return res


def test_every_case_is_listed(rows):
    assert sorted(NAMES) == sorted(rows)


@pytest.mark.parametrize("name", NAMES)
def test_standard_rows(fa, rows, name):
    a, chosen = rows[name]
    for top_n in lc.TOPS:
        if top_n <= a.shape[1]:
            check(fa, a, chosen, top_n, name)


@pytest.mark.parametrize("V", [4099, 32000])
def test_rank_extremes_and_ties(fa, V):
    rs = np.random.RandomState(77)
    a = (2.0 * rs.standard_normal((6, V))).astype(np.float32)
    ties = np.sort(rs.choice(V, 20, replace=False))
    a[2, ties] = np.float32(1.25)                                       # a block of 20 ties inside the row, scored at its first and last index
    a[3] = a[2]
    a[1, 17] = a[1].min() - 1.0                                         # a unique minimum
    ninf = rs.choice(V, 50, replace=False)
    a[4, ninf] = -np.inf
    targets = [int(np.argmax(a[0])), 17, int(ties[0]), int(ties[-1]), int(ninf[7]), int(np.argmax(a[5]))]
    for top_n in (0, 20):
        res = check(fa, a, targets, top_n, "extremes_%d" % V)
        assert int(res.target_rank[0]) == 1 and int(res.target_rank[1]) == V
        assert int(res.target_rank[3]) - int(res.target_rank[2]) == 19
        assert res.target_logprob[4] == -np.inf and 1 <= int(res.target_rank[4]) <= V


def test_rows_without_a_target_and_mixed_blocks(fa):
    rs = np.random.RandomState(78)
    V = 32001
    a = (2.0 * rs.standard_normal((5, V))).astype(np.float32)
    for targets in ([NO], [NO, 5, NO, V - 1, NO], [NO] * 5):
        for top_n in (0, 5):
            res = check(fa, a[:len(targets)], targets, top_n, "no_target")
            for t, g in enumerate(targets):
                assert (g == NO) == bool(np.isnan(res.target_logprob[t])) and (g == NO) == (int(res.target_rank[t]) == 0)


def test_more_rows_than_compute_units(fa):
    rs = np.random.RandomState(79)
    T, V = 300, 4099
    a = (2.0 * rs.standard_normal((T, V))).astype(np.float32)
    targets = rs.randint(0, V, T).astype(np.uint32)
    targets[::7] = NO
    check(fa, a, targets, 5, "t300")


def test_top_n_equal_to_the_vocabulary(fa, rows):
    a, chosen = rows["normal_20_1"]
    res = check(fa, a, chosen, 20, "v20")
    assert sorted(res.top_ids[0].tolist()) == list(range(20))
    assert int(res.top_ids[0][int(res.target_rank[0]) - 1]) == int(chosen[0])


@pytest.mark.parametrize("name", ["normal_4099_3", "normal_32001_2", "normal_152064_1", "top_ties", "neg_inf", "underflow", "t64"])
def test_same_arithmetic_as_the_logprob_kernel(fa, rows, name):
    """One device header serves both kernels: on the same rows and tokens the values agree bit for bit."""
    a, chosen = rows[name]
    for top_n in (0, 20):
        tok, ids, lps = fa.op_logprobs(a, chosen, top_n)
        res = fa.op_score(a, chosen, top_n)
        assert np.array_equal(tok.view(np.uint32), res.target_logprob.view(np.uint32)), name
        assert np.array_equal(ids, res.top_ids) and np.array_equal(lps.view(np.uint32), res.top_logprobs.view(np.uint32)), name
