"""The log-prob kernel alone (fl_op_logprobs) against numpy float64 on the same fp32 rows: values within the derived tolerance of
tests/logprob_cases.py, top ids EXACTLY np.lexsort((idx, -x))[:top_n].  (The entry launches the kernel twice and fails if the two
results differ.)"""
import numpy as np
import pytest

import logprob_cases as lc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fa():
    import fastllm_amd
    assert fastllm_amd.device_count() >= 1
    return fastllm_amd


@pytest.fixture(scope="module")
def rows():
    return lc.rows()


NAMES = ["normal_31_1", "normal_4099_3", "normal_32000_2", "normal_32001_2", "normal_152064_1", "normal_20_1", "flat", "ramp_up", "ramp_down",
         "top_one_lane_32000", "top_one_lane_32001", "top_one_lane_vec", "top_tail_32000", "top_tail_32001", "top_tail_4099", "top_ties", "underflow", "neg_inf", "t64"]


def test_every_case_is_listed(rows):
    assert sorted(NAMES) == sorted(rows)


@pytest.mark.parametrize("name", NAMES)
def test_rows_against_float64(fa, rows, name):
    a, chosen = rows[name]
    T, V = a.shape
    for top_n in lc.TOPS:
        if top_n > V:
            continue
        tok, ids, lps = fa.op_logprobs(a, chosen, top_n)
        assert ids.shape == (T, top_n) and lps.shape == (T, top_n) and tok.shape == (T,)
        for t in range(T):
            lc.check_row(a[t], chosen[t], top_n, tok[t], ids[t], lps[t], what=(name, top_n, t))


def test_top_n_equal_to_the_vocabulary(fa, rows):
    a, chosen = rows["normal_20_1"]
    tok, ids, lps = fa.op_logprobs(a, chosen, 20)
    assert sorted(ids[0].tolist()) == list(range(20))
    lc.check_row(a[0], chosen[0], 20, tok[0], ids[0], lps[0])


def test_flat_row_values(fa, rows):
    a, chosen = rows["flat"]
    tok, ids, lps = fa.op_logprobs(a, chosen, 20)
    assert ids[0].tolist() == list(range(20))
    assert np.abs(lps[0] + np.log(a.shape[1])).max() <= 2.0 ** -20 * (1 + np.log(a.shape[1])) and abs(tok[0] + np.log(a.shape[1])) <= 2.0 ** -19


def test_gather_overflow_falls_back_to_ranking(fa):
    """V beyond kLpKeys * 1024 / 20: twenty lanes whose every element beats every other lane's maximum overflow the LDS gather, and
    the row is ranked by masked maxima instead.  The result is the same order."""
    V = 1024 * 450 + 4                                              # 16-byte path: lane l holds chunks l + 1024 k
    rs = np.random.RandomState(77)
    a = rs.standard_normal((1, V)).astype(np.float32)
    chunk = np.arange(V) // 4
    hot = (chunk % 1024) < 20
    a[0, hot] += 100.0
    tok, ids, lps = fa.op_logprobs(a, [5], 20)
    lc.check_row(a[0], 5, 20, tok[0], ids[0], lps[0], what="overflow")
    b = rs.standard_normal((1, V - 1)).astype(np.float32)           # ... and on the scalar path (V % 4 != 0: lane l holds l + 1024 k)
    b[0, (np.arange(V - 1) % 1024) < 20] += 100.0
    tok, ids, lps = fa.op_logprobs(b, [5], 20)
    lc.check_row(b[0], 5, 20, tok[0], ids[0], lps[0], what="overflow scalar")


def test_rows_are_independent_of_their_neighbours(fa, rows):
    a, chosen = rows["t64"]
    perm = np.random.RandomState(5).permutation(a.shape[0])
    t0, i0, l0 = fa.op_logprobs(a, chosen, 5)
    t1, i1, l1 = fa.op_logprobs(a[perm], np.asarray(chosen)[perm], 5)
    assert np.array_equal(t1, t0[perm]) and np.array_equal(i1, i0[perm]) and np.array_equal(l1, l0[perm])
