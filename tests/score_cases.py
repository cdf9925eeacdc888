"""What the scoring tests (tests/test_gpu_score_ops.py, test_gpu_score.py, test_gpu_score_packed.py) share on top of the log-prob rows,
reference and tolerance of tests/logprob_cases.py, which they use unchanged: the rank of a target, and the checks of one scored row."""
import numpy as np

import logprob_cases as lc  # noqa: F401  (re-exported: the rows, ref_logprobs, tol and check_row)

NO_TARGET = 0xFFFFFFFF


def ref_rank(x, t):
    """1 + the position of id t in the order "logit descending, lower index first" of the fp32 row x."""
    x = np.asarray(x, dtype=np.float32)
    order = np.lexsort((np.arange(x.size), -x))
    return int(np.flatnonzero(order == int(t))[0]) + 1


def check_scored_row(x, target, top_n, res, t, what=""):
    """Row t of a ScoreResult against the fp32 row x the kernel read: lc.check_row for the target's log-prob and the tops, the rank
    exactly; a row without a target reports NaN and rank 0, and its tops all the same."""
    if int(target) == NO_TARGET:
        assert np.isnan(res.target_logprob[t]) and int(res.target_rank[t]) == 0, (what, t, res.target_logprob[t], res.target_rank[t])
        lp, _ = lc.ref_logprobs(x)
        c = int(np.argmax(lp))                                         # (any finite entry: only the tops are checked)
        lc.check_row(x, c, top_n, lp[c], res.top_ids[t], res.top_logprobs[t], what=(what, t, "no target"))
        return
    lc.check_row(x, target, top_n, res.target_logprob[t], res.top_ids[t], res.top_logprobs[t], what=(what, t))
    r = ref_rank(x, target)
    assert int(res.target_rank[t]) == r, (what, t, "rank", int(res.target_rank[t]), r)
    if r <= top_n:
        assert int(res.top_ids[t][r - 1]) == int(target), (what, t)


def next_targets(ids):
    """The default targets of a sequence: the next id, none for the last row."""
    ids = np.asarray(ids, dtype=np.uint32)
    return np.concatenate([ids[1:], [NO_TARGET]]).astype(np.uint32)
