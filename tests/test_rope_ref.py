"""tests/rope_ref.py checked on the CPU: against tests/decoder_ref.py's RoPE, its exact and its float64 rotation against each other, the
cache placement in both value layouts, and the bound of the fused forms -- the reference alone, run in float32 in two summation orders
on the inputs of tests/test_gpu_rope_ops.py, stays inside it, and a position off by one, a neighbouring row's 1/rms and a missing bias
do not."""
import numpy as np
import pytest

import decoder_ref
import norm_ref
import rope_ref as R

HEADS = [(4, 2, 64), (2, 1, 128), (3, 1, 64), (2, 2, 128)]


def test_tables_and_rotation_agree_with_decoder_ref():
    H, Hkv, d, T, pos0 = 4, 2, 64, 7, 3
    cfg = dict(hidden_size=H * d, num_attention_heads=H, rope_theta=R.THETA)
    cos, sin = R.tables(pos0 + T, d)
    c64, s64 = decoder_ref.rope_tables(cfg, pos0 + T)
    np.testing.assert_array_equal(cos.astype(np.float64), c64)
    np.testing.assert_array_equal(sin.astype(np.float64), s64)
    y = np.random.RandomState(1).standard_normal((T, (H + 2 * Hkv) * d))
    pos = pos0 + np.arange(T)
    (q, k, v), _ = R.rotate64(y, cos, sin, pos, H, Hkv, d)
    c, s = c64[pos][:, None, :], s64[pos][:, None, :]

    def rope(a):                                             # decoder_ref.hidden_states' closure, restated: [T, heads, d], rotate-half
        a1, a2 = a[..., :d // 2], a[..., d // 2:]
        return np.concatenate([a1 * c - a2 * s, a2 * c + a1 * s], axis=-1)

    np.testing.assert_allclose(q, rope(y[:, :H * d].reshape(T, H, d)).reshape(T, -1), rtol=0, atol=1e-15)
    np.testing.assert_allclose(k, rope(y[:, H * d:(H + Hkv) * d].reshape(T, Hkv, d)).reshape(T, -1), rtol=0, atol=1e-15)
    np.testing.assert_array_equal(v, y[:, (H + Hkv) * d:])


def test_sum_slabs_order():
    """slab by slab in slab order, then the bias: with 2^24, 1, -2^24 the order shows"""
    qkv = np.array([[[2.0 ** 24]], [[1.0]], [[-2.0 ** 24]]], np.float32)
    assert R.sum_slabs(qkv)[0, 0] == 0.0                     # (2^24 + 1) rounds to 2^24 first
    assert R.sum_slabs(qkv[[0, 2, 1]])[0, 0] == 1.0
    assert R.sum_slabs(qkv, np.array([0.5], np.float32))[0, 0] == 0.5


@pytest.mark.parametrize("H,Hkv,d", HEADS)
def test_rotate_exact_within_the_bound_of_rotate64(H, Hkv, d):
    """from the SAME float32 values the exact rotation is three roundings from the float64 one: far inside the fused bound"""
    T = 9
    x, _ = R.qkv_inputs(1, T, (H + 2 * Hkv) * d, 5, False)
    cos, sin = R.tables(40, d)
    pos = 11 + np.arange(T)
    for dtype in ("bf16", "f32"):
        got = R.rotate_exact(x[0], cos, sin, pos, H, Hkv, d, dtype)
        want, lims = R.fused_bounds(x[0].astype(np.float64), cos, sin, pos, H, Hkv, d, 256, dtype)
        for g, w, lim in zip(got, want, lims):
            assert (np.abs(R.widen(g) - w) <= lim).all()
        if dtype == "f32":                                   # three roundings of 2^-24 on values below |a| + |b|
            _, (mq, mk) = R.rotate64(x[0].astype(np.float64), cos, sin, pos, H, Hkv, d)
            assert (np.abs(got[0] - want[0]) <= 3 * 2.0 ** -24 * 2 * mq).all() and (np.abs(got[1] - want[1]) <= 3 * 2.0 ** -24 * 2 * mk).all()
            np.testing.assert_array_equal(got[2], want[2])


def test_half_ulp_is_what_rounding_needs():
    """The bf16 term of the bound is half an ulp, 2^-8 * 2^floor(log2 |r|): the correctly rounded value of a float32 number reaches it
    (ties) and never exceeds it, while half of that figure (2^-9 * 2^e, a quarter ulp) is missed by a third of random values -- no
    kernel and no reference could meet it, at any scale of the inputs."""
    import synth
    assert R.half_ulp_bf16(1.0) == 2.0 ** -8 and R.half_ulp_bf16(-3.5) == 2.0 ** -7 and R.half_ulp_bf16(0.0) == 0.0
    tie = np.array([1.0 + 2.0 ** -8], np.float32)
    assert abs(float(synth.bf16_bits_to_f32(synth.f32_to_bf16_bits(tie))[0]) - float(tie[0])) == R.half_ulp_bf16(tie)[0]
    x = (np.random.RandomState(0).standard_normal(100000) * 8).astype(np.float32)
    err = np.abs(synth.bf16_bits_to_f32(synth.f32_to_bf16_bits(x)).astype(np.float64) - x)
    assert (err <= R.half_ulp_bf16(x)).all()
    assert (err > R.half_ulp_bf16(x) / 2).mean() > 0.3


@pytest.mark.parametrize("vt", [0, 1])
@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_place_round_trips(vt, dtype):
    layers, Hkv, sa, d, layer = 2, 2, 12, 8, 1
    ck, cv = R.new_caches(layers, Hkv, sa, d, vt, dtype, 3)
    assert cv.shape == ((layers, Hkv, d, sa) if vt else (layers, Hkv, sa, d))
    assert len(np.unique(ck)) > 100 and (R.widen(ck) >= 1).all() and (R.widen(ck) < 2).all()     # the pattern: many values, all in [1, 2)
    rs = np.random.RandomState(4)
    slot = np.array([3, 4, 11])
    k = rs.randint(1, 1000, size=(3, Hkv * d)).astype(ck.dtype)
    v = rs.randint(1, 1000, size=(3, Hkv * d)).astype(ck.dtype)
    nk, nv = R.place(ck, cv, k, v, slot, vt, layer)
    np.testing.assert_array_equal(nk[layer][:, slot, :].transpose(1, 0, 2).reshape(3, -1), k)
    got_v = nv[layer][:, :, slot].transpose(2, 0, 1) if vt else nv[layer][:, slot, :].transpose(1, 0, 2)
    np.testing.assert_array_equal(got_v.reshape(3, -1), v)
    mk, mv = R.appended_mask(ck, slot, vt, layer)
    assert mk.sum() == mv.sum() == 3 * Hkv * d and mv.shape == cv.shape
    np.testing.assert_array_equal(nk[~mk], ck[~mk])          # everything else is the pattern, the other layer included
    np.testing.assert_array_equal(nv[~mv], cv[~mv])
    assert (nk[mk] != ck[mk]).all() and (nv[mv] != cv[mv]).all()
    np.testing.assert_array_equal(nk[0], ck[0])


def _float32_projections(c):
    """the reference's own projection in float32, in two summation orders: forward, and K split in four slabs summed in slab order"""
    xs, W, inv = c["xs"].astype(np.float32), c["Wv"].astype(np.float32), c["inv"].astype(np.float32)[:, None]
    b = c["b"] if c["b"] is not None else np.float32(0)
    K = xs.shape[1]
    fwd = np.zeros((xs.shape[0], W.shape[0]), np.float32)
    for k in range(K):                                       # strictly left to right
        fwd = (fwd + xs[:, k:k + 1] * W[:, k][None, :]).astype(np.float32)
    q = K // 4
    slabs = np.zeros_like(fwd)
    for s in range(4):
        slabs = (slabs + (xs[:, s * q:(s + 1) * q] @ W[:, s * q:(s + 1) * q].T).astype(np.float32)).astype(np.float32)
    return [(y * inv + b).astype(np.float32) for y in (fwd, slabs)]


# every K of the fused GPU cases (their inputs are rope_ref.fused_inputs' too), on a prompt's rows, a batch's and a single row
@pytest.mark.parametrize("T,K", [(34, 256), (20, 512), (20, 1024), (33, 1536), (8, 1536), (1, 256), (1, 1536)])
@pytest.mark.parametrize("H,Hkv,d", HEADS)
@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_the_reference_stays_inside_the_fused_bound_and_errors_do_not(T, K, H, Hkv, d, dtype):
    c = R.fused_inputs(T, K, H, Hkv, d, 2, True, dtype, 77 + T + K + H)
    cos, sin = R.tables(T + 8, d)
    pos = 5 + np.arange(T)
    want, lims = R.fused_bounds(c["y"], cos, sin, pos, H, Hkv, d, K, dtype)
    for y32 in _float32_projections(c):
        got = R.rotate_exact(y32, cos, sin, pos, H, Hkv, d, dtype)
        for g, w, lim in zip(got, want, lims):
            assert (np.abs(R.widen(g) - w) <= lim).all(), float((np.abs(R.widen(g) - w) / lim).max())
    # ... and the bound separates the errors a fused form can make, at pair j = 0 of at least one q head and one k head of every row
    half = d // 2
    j0 = lambda a, heads: a.reshape(T, heads, d)[:, :, [0, half]]                   # noqa: E731

    def caught(y_wrong, pos_wrong):
        (wq, wk, _), _ = R.rotate64(y_wrong, cos, sin, pos_wrong, H, Hkv, d)
        badq = (np.abs(j0(wq, H) - j0(want[0], H)) > j0(lims[0], H)).any(axis=2)
        badk = (np.abs(j0(wk, Hkv) - j0(want[1], Hkv)) > j0(lims[1], Hkv)).any(axis=2)
        return badq.any(axis=1) & badk.any(axis=1)

    assert caught(c["y"], pos + 1).all()                                             # a position off by one: a radian at j = 0
    y_nobias = c["y"] - c["b"].astype(np.float64)
    assert caught(y_nobias, pos).all()                                               # a missing bias
    if T > 1:                                                                        # a neighbouring row's 1/rms: a power of two off
        inv_nb = np.roll(c["inv"], 1)                                                # (row 0 takes the last row's: rows 1 .. T-1 count)
        assert (np.maximum(inv_nb / c["inv"], c["inv"] / inv_nb)[1:] > 1.5).all()
        assert caught(norm_ref.project(c["xs"], inv_nb, c["Wv"], c["b"]), pos)[1:].all()
