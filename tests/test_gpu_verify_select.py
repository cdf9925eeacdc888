"""The selection kernel of the verify step alone (fl_op_verify_select): per row the LAST maximal index, exactly numpy's on the same
array, and the acceptance scan over the drafted ids.  (The entry launches the kernel twice and fails if the second launch, which
meets the arrival ticket the first one put back, answers differently.)"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

VS = [1, 63, 1025, 32000, 152064]
TS = [1, 2, 16]


@pytest.fixture(scope="module")
def fa():
    import fastllm_amd
    assert fastllm_amd.device_count() >= 1
    return fastllm_amd


def argmax_last(a):
    """numpy: the last index of each row's maximum."""
    return (a.shape[1] - 1 - np.argmax(a[:, ::-1], axis=1)).astype(np.uint32)


def scan(draft, am):
    n = 0
    while n < len(draft) and draft[n] == am[n]:
        n += 1
    return n


def logits_for(T, V, seed):
    rs = np.random.RandomState(seed)
    a = rs.standard_normal((T, V)).astype(np.float32)
    if V > 1:
        a[0, 0] = a[0, V - 1] = 9.0                      # an exact tie of the maximum at the first and the last index
        if T > 1:
            a[1, V - 1] = 11.0                           # the maximum is the row's last element
        if T > 2:
            a[2, 0] = 11.0                               # ... and its first
            a[3, [V // 3, V // 2]] = 12.0                # a tie inside the row
            a[T - 1, V // 2] = np.inf
    return a


@pytest.mark.parametrize("V", VS)
@pytest.mark.parametrize("T", TS)
def test_argmax_and_acceptance(fa, T, V):
    a = logits_for(T, V, 7 * T + V)
    want = argmax_last(a)
    if V > 1:
        assert want[0] == V - 1 and (T < 2 or want[1] == V - 1) and (T < 3 or (want[2] == 0 and want[3] == V // 2))
    other = lambda t: (int(want[t]) + 1) % V if V > 1 else None      # a wrong id for row t
    drafts = [want[: T - 1].copy()]                                    # all right
    if T > 1 and V > 1:
        d = want[: T - 1].copy(); d[0] = other(0); drafts.append(d)    # wrong at 0 (everything after it is right and must not count)
        d = want[: T - 1].copy(); d[T - 2] = other(T - 2); drafts.append(d)     # wrong at the last position
    if T > 2 and V > 1:
        d = want[: T - 1].copy(); d[4] = other(4); drafts.append(d)    # right after a wrong one
        d = np.array([other(t) for t in range(T - 1)], np.uint32); drafts.append(d)    # all wrong
    for d in drafts:
        am, n = fa.op_verify_select(a, d)
        assert np.array_equal(am, want), (T, V, np.flatnonzero(am != want))
        assert n == scan(d, want), (T, V, d, n)
    if T > 1 and V > 1:
        assert [scan(d, want) for d in drafts[:3]] == [T - 1, 0, T - 2]
    if T > 2 and V > 1:
        assert scan(drafts[3], want) == 4


def test_rows_are_independent_of_their_neighbours(fa):
    """Row t's id comes from row t alone: permuting the rows permutes the ids (a wrong row stride would not)."""
    V, T = 1025, 16
    a = logits_for(T, V, 99)
    perm = np.random.RandomState(5).permutation(T)
    am0, _ = fa.op_verify_select(a, np.zeros(T - 1, np.uint32))
    am1, _ = fa.op_verify_select(a[perm], np.zeros(T - 1, np.uint32))
    assert np.array_equal(am1, am0[perm]) and np.array_equal(am0, argmax_last(a))
