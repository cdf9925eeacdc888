"""pool_rows_kernel ALONE, through fl_op_pool_rows: the pooled final hidden states of a pack against a numpy float32 restatement
(decoder_ref.hid_f32 / pool_f32: hid = (x * inv_rms) * w, both products rounded; MEAN adds the rows in order from +0 and divides
once by the count).  Unnormalised outputs must equal the restatement BIT FOR BIT; normalised ones are compared with the float64
normalisation of those exact fp32 vectors under relative error 2 * dims * 2^-24 (decoder_ref.check_normalized: derived, not measured).
Shapes: h 64 (a quarter of one column chunk), 264 (one chunk and 8 columns; 66 lanes' worth of vectors) and 4096 (16 chunks);
members of 1, 2, 17 and 300 rows (one row, fewer rows than the sixteen the kernel requests ahead, one more, and many rounds); dimensions 1 and 37
make output rows that start off a 16-byte boundary and lanes whose four columns straddle the end.  The output is pre-filled with the
0xff pattern by the entry point, so an element the kernel does not write shows up as NaN."""
import numpy as np
import pytest

import decoder_ref

pytestmark = pytest.mark.gpu

COUNTS = [1, 2, 17, 300]
HS = [64, 264, 4096]
POOLINGS = ["last", "first", "mean", "none"]


@pytest.fixture(scope="module")
def fa():
    import fastllm_amd
    assert fastllm_amd.device_count() >= 1
    return fastllm_amd


_CASES = {}


def case(h):
    """x [320, h], inv_rms [320], w [h] and the restated hidden states -- made once per h, never modified"""
    if h not in _CASES:
        rs = np.random.RandomState(77 + h)
        T = sum(COUNTS)
        x = rs.standard_normal((T, h)).astype(np.float32)
        inv = rs.uniform(0.5, 2.0, T).astype(np.float32)
        w = (1.0 + 0.1 * rs.standard_normal(h)).astype(np.float32)
        _CASES[h] = (x, inv, w, decoder_ref.hid_f32(x, inv, w))
    return _CASES[h]


def dims_of(h):
    return [0, 1, 37, h]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("pooling", POOLINGS)
@pytest.mark.parametrize("h", HS)
def test_pooled_vectors_equal_the_restatement(fa, h, pooling):
    x, inv, w, hid = case(h)
    for dims in dims_of(h):
        want = decoder_ref.pool_f32(hid, COUNTS, pooling, dims)
        got = fa.op_pool_rows(x, inv, w, COUNTS, pooling=pooling, normalize=False, dimensions=dims)
        assert got.shape == want.shape
        assert not np.isnan(got).any(), "h %d dims %d %s: an element keeps the 0xff pattern" % (h, dims, pooling)
        assert np.array_equal(bits(got), bits(want)), "h %d dims %d %s: %d elements differ, max %g" % (
            h, dims, pooling, int((bits(got) != bits(want)).sum()), np.abs(got - want).max())
        norm = fa.op_pool_rows(x, inv, w, COUNTS, pooling=pooling, normalize=True, dimensions=dims)
        assert norm.shape == want.shape and not np.isnan(norm).any()
        decoder_ref.check_normalized(norm, want, "h %d dims %d %s" % (h, dims, pooling))


@pytest.mark.parametrize("pooling", POOLINGS)
def test_a_zero_member_gives_zeros(fa, pooling):
    x, inv, w, _ = case(264)
    x = x.copy()
    x[3:20] = 0.0                                              # the member of 17 rows
    for normalize in (False, True):
        got = fa.op_pool_rows(x, inv, w, COUNTS, pooling=pooling, normalize=normalize, dimensions=37)
        zero = got[3:20] if pooling == "none" else got[2:3]
        assert np.isfinite(got).all() and (zero == 0.0).all()
        assert (np.abs(got[:3] if pooling == "none" else got[:2]).max(axis=1) > 0).all()      # the neighbours are not


@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("pooling", ["last", "first", "mean"])
@pytest.mark.parametrize("h", HS)
def test_a_member_does_not_depend_on_the_pack(fa, h, pooling, normalize):
    x, inv, w, _ = case(h)
    off = np.concatenate([[0], np.cumsum(COUNTS)])
    n = len(COUNTS)

    def run(order):
        rows = np.concatenate([np.arange(off[i], off[i + 1]) for i in order])
        got = fa.op_pool_rows(x[rows], inv[rows], w, [COUNTS[i] for i in order], pooling=pooling, normalize=normalize, dimensions=37 if h == 264 else 0)
        return {i: bits(got[k]).tobytes() for k, i in enumerate(order)}

    full, again = run(list(range(n))), run(list(range(n)))
    moved, rot = run(list(range(n))[::-1]), run([(i + 1) % n for i in range(n)])
    for i in range(n):
        assert full[i] == again[i], "member %d: two runs of the same launch differ" % i
        assert full[i] == moved[i] == rot[i], "member %d changes with its place in the pack" % i
        assert run([i])[i] == full[i], "member %d differs alone" % i


def test_every_row_is_its_own_member_with_none(fa):
    """NONE over the pack equals LAST over members of one row each"""
    x, inv, w, _ = case(264)
    for normalize in (False, True):
        none = fa.op_pool_rows(x, inv, w, COUNTS, pooling="none", normalize=normalize)
        last = fa.op_pool_rows(x, inv, w, [1] * x.shape[0], pooling="last", normalize=normalize)
        assert np.array_equal(bits(none), bits(last))


def test_bad_shapes_are_refused(fa):
    import ctypes as C
    x, inv, w, _ = case(64)
    out = np.zeros((4, 64), np.float32)
    off = np.array([0, 1, 3, 20, 320], np.uint64)
    for e in (fa.make_embed(dimensions=65), fa.make_embed(pooling=4), fa.make_embed(normalize=2)):
        assert fa.lib().fl_op_pool_rows(x.ctypes.data, inv.ctypes.data, w.ctypes.data, off.ctypes.data, 4, 64, C.byref(e), out.ctypes.data) == -8
    assert (out == 0).all()
