"""Rows, float64 reference and the derived tolerance shared by the log-prob tests (tests/test_gpu_logprobs_ops.py, tests/test_gpu_logprobs.py,
tests/test_logprobs_abi.py)."""
import numpy as np

TOPS = [0, 1, 5, 20]


def ref_logprobs(x):
    """float64 log-softmax of one fp32 row and the stable order "logit descending, lower index first"."""
    x = np.asarray(x, dtype=np.float32)
    x64 = x.astype(np.float64)
    m = x64.max()
    with np.errstate(divide="ignore", invalid="ignore"):
        lp = (x64 - m) - np.log(np.exp(x64 - m).sum())
    order = np.lexsort((np.arange(x.size), -x))
    return lp, order


def tol(x, lp):
    """tol_i = 2**-20 * (1 + |x_i - m| + |lp_i|): four times the first-order rounding bound of the prescribed arithmetic -- one fp32
    subtraction (2**-24 |x_i - m|), expf within 2 ulp and an fp64 sum (2**-22 relative on the sum, i.e. absolute on its log), an fp32
    log and the final fp32 subtraction (2**-24 |lp_i| each).  -inf entries have lp = -inf exactly; their tolerance is irrelevant."""
    x64 = np.asarray(x, dtype=np.float64)
    d = np.abs(x64 - x64.max())
    d[~np.isfinite(d)] = 0.0
    a = np.abs(lp)
    a[~np.isfinite(a)] = 0.0
    return 2.0 ** -20 * (1.0 + d + a)


def f32_restatement(x):
    """The kernel's arithmetic restated in numpy: fp32 subtraction, fp32 exp, fp64 sum, fp32 log and subtraction."""
    x = np.asarray(x, dtype=np.float32)
    m = x.max()
    with np.errstate(invalid="ignore", divide="ignore"):
        d = (x - m).astype(np.float32)
        s = np.exp(d).astype(np.float32).astype(np.float64).sum()
        lz = np.float32(np.log(s))
        return ((d - lz).astype(np.float32)).astype(np.float64)


def check_row(x, chosen, top_n, got_tok, got_ids, got_lps, what=""):
    """One row's results against the float64 reference: values within tol, ids exactly."""
    lp, order = ref_logprobs(x)
    t = tol(x, lp)
    c = int(chosen)
    if np.isfinite(lp[c]):
        assert abs(float(got_tok) - lp[c]) <= t[c], (what, "chosen", c, float(got_tok), lp[c], t[c])
    else:
        assert float(got_tok) == lp[c], (what, "chosen", c, float(got_tok), lp[c])
    want = order[:top_n]
    assert np.array_equal(np.asarray(got_ids[:top_n], dtype=np.int64), want), (what, "ids", got_ids[:top_n], want)
    for j, i in enumerate(want):
        if np.isfinite(lp[i]):
            assert abs(float(got_lps[j]) - lp[i]) <= t[i], (what, "rank", j, int(i), float(got_lps[j]), lp[i], t[i])
        else:
            assert float(got_lps[j]) == lp[i], (what, "rank", j, int(i), float(got_lps[j]), lp[i])


def place_top(x, idx, rs):
    """The 20 largest values of the row, distinct, at the given indices."""
    top = float(x.max())
    vals = (top + 1.0 + rs.permutation(len(idx)) * 0.25).astype(np.float32)
    x[np.asarray(idx)] = vals
    return x


def rows():
    """name -> (logits [T, V], chosen [T]); seeded."""
    out = {}
    rs = np.random.RandomState(1234)
    normal = lambda T, V: (2.0 * rs.standard_normal((T, V))).astype(np.float32)     # N(0, 4)
    for V, T in ((31, 1), (4099, 3), (32000, 2), (32001, 2), (152064, 1), (20, 1)):
        a = normal(T, V)
        out["normal_%d_%d" % (V, T)] = (a, rs.randint(0, V, T))
    V = 32000
    out["flat"] = (np.full((1, V), 1.5, np.float32), [V - 1])
    out["ramp_up"] = ((np.arange(V, dtype=np.float32) * 1e-3)[None, :].copy(), [0])
    out["ramp_down"] = ((np.arange(V, dtype=np.float32)[::-1] * 1e-3)[None, :].copy(), [V - 1])
    for VV in (V, 32001):                                                            # one lane's stride of the scalar path (V % 4 != 0)
        a = normal(1, VV)
        place_top(a[0], [k * 1024 + 7 for k in range(20)], rs)
        out["top_one_lane_%d" % VV] = (a, [7])
    a = normal(1, V)                                                                  # ... and of the 16-byte path: five whole chunks of lane 7
    place_top(a[0], [4 * (7 + 1024 * k) + j for k in range(5) for j in range(4)], rs)
    out["top_one_lane_vec"] = (a, [28])
    for VV in (V, 32001, 4099):
        a = normal(1, VV)
        place_top(a[0], list(range(VV - 23, VV - 3)), rs)
        out["top_tail_%d" % VV] = (a, [VV - 4])
    a = normal(1, V)
    ties = np.sort(rs.choice(V, 20, replace=False))
    a[0, ties] = float(a.max()) + 3.0
    out["top_ties"] = (a, [int(ties[-1])])                                            # (ArgMax's choice: the LAST maximal index)
    a = np.full((1, V), -80.0, np.float32)
    a[0, 12345] = 0.0
    a[0, ::97] += rs.standard_normal(len(a[0, ::97])).astype(np.float32) * 0.5
    a[0, 12345] = 0.0
    out["underflow"] = (a, [3])
    a = normal(1, V)
    ninf = rs.choice(V, 1000, replace=False)
    a[0, ninf] = -np.inf
    out["neg_inf"] = (a, [int(ninf[0])])
    out["t64"] = (normal(64, 4099), rs.randint(0, 4099, 64))
    return out
