"""The 65-128-row MXFP4 weight stream (k_gemm_rows128_w4.hip) alone, through fl_op_linear_w4_tall, against numpy on mx4_values(q, e):
bit for bit where fp32 sums are exact, fp64 numpy otherwise.  The cases and bounds are those of tests/test_gpu_linear_w4_wide_ops.py."""
import numpy as np
import pytest

import synth
from test_w4_abi import mx4_values, quantize_mx4_ref

pytestmark = pytest.mark.gpu

# one block, a partial row group; an odd group count and a partial pair of x stages; many stages; K slices
SHAPES = [(3, 32), (33, 1056), (129, 4608), (129, 14368)]
# one row in a fifth token tile, an odd count of full tiles, a ragged last tile, the full height ... and Mistral-7B's QKV
CASES = [(T, N, K) for T in (65, 80, 113, 128) for N, K in SHAPES] + [(128, 6144, 4096)]
INT_CODE = np.array([8 | 4, 8 | 2, 0, 2, 4], dtype=np.uint8)                                  # integers -2..2 as e2m1 codes


@pytest.fixture(scope="module")
def fa():
    import fastllm_amd
    assert fastllm_amd.device_count() >= 1
    return fastllm_amd


def bf16(a):
    return synth.f32_to_bf16_bits(np.asarray(a, dtype=np.float32))


def pack(codes):
    return (codes[:, 0::2] | codes[:, 1::2] << 4).astype(np.uint8)


@pytest.mark.parametrize("T,N,K", CASES)
def test_bit_exact_on_small_operands(fa, T, N, K):
    """Every code of both signs under block exponents -1..1, x integers in -2..2, row scales powers of two: a term is a multiple of
    2^-2 of at most 24, so every partial sum stays below 2^24 quanta in any order -- over lanes, MFMAs, x stages and K slabs -- and
    the result equals numpy bit for bit."""
    rs = np.random.RandomState(T * 131 + N * 7 + K)
    q, e = rs.randint(0, 256, size=(N, K // 2)).astype(np.uint8), (127 + rs.randint(-1, 2, size=(N, K // 32))).astype(np.uint8)
    xi = rs.randint(-2, 3, size=(T, K))
    r = np.ldexp(np.float32(1.0), rs.randint(-2, 3, size=T)).astype(np.float32)
    assert 96 * K + 2 ** 7 < 2 ** 24
    if (N, K) == (129, 14368):
        assert fa.op_linear_w4_tall_plan(T, N, K) > 1
    ref = (xi.astype(np.float64) @ mx4_values(q, e).T.astype(np.float64)) * r[:, None]
    np.testing.assert_array_equal(fa.op_linear_w4_tall(bf16(xi), q, e, row_scale=r), ref.astype(np.float32))


@pytest.mark.parametrize("row", [0, 64, 112])
@pytest.mark.parametrize("col", [0, 1, 9, 18, 27, 37, 101, 135, 515, 1055])
def test_converts_every_code_at_every_place(fa, col, row):
    """All 16 codes against a one-hot x (both nibbles, all four dwords of a load, both blocks of a lane = both stages of a pair,
    every lane group, the second pair, the second scale group, the last column of a ragged K; the first row, the first row of the
    fifth token tile and the last row of a ragged eighth), block scales alternating from 2^-120, 2^0 and 2^100: y = 2^e * value(code)
    exactly in the hot row, exactly 0 in the others."""
    N, K, T = 48, 1056, 113                                     # weight row 16 i + c: code c under the i-th base exponent
    codes, x = np.zeros((N, K), dtype=np.uint8), np.zeros((T, K), dtype=np.float32)
    codes[:, col], x[row, col] = np.arange(N) & 15, 1.0
    e = (127 + np.repeat([-120, 0, 100], 16)[:, None] + (np.arange(K // 32) & 1)[None, :]).astype(np.uint8)
    want = np.zeros((T, N), dtype=np.float32)
    want[row] = mx4_values(pack(codes), e)[:, col]
    np.testing.assert_array_equal(fa.op_linear_w4_tall(bf16(x), pack(codes), e), want)


@pytest.mark.parametrize("T,N,K", CASES)
def test_random_operands(fa, T, N, K):
    """Random weights through the quantiser's restatement, N(0,1) x and row scales, against fp64 numpy on 2^e * q: the bound of
    tests/test_gpu_linear_w4_ops.py::test_random_operands."""
    rs = np.random.RandomState(N + 3 * K + T)
    q, e = quantize_mx4_ref((rs.standard_normal((N, K)) * 0.05).astype(np.float32))
    xb, r = bf16(rs.standard_normal((T, K))), rs.standard_normal(T).astype(np.float32)
    ref = (synth.bf16_bits_to_f32(xb).astype(np.float64) @ mx4_values(q, e).astype(np.float64).T) * r[:, None].astype(np.float64)
    np.testing.assert_allclose(fa.op_linear_w4_tall(xb, q, e, row_scale=r), ref, atol=2e-5 * np.sqrt(K) + 1e-5, rtol=1e-5)


@pytest.mark.parametrize("T", [65, 128])
@pytest.mark.parametrize("I,K", [(40, 64), (24, 1056), (352, 256)])
def test_silu_gate_on_small_integers(fa, I, K, T):
    """gate | up rows in HF order in, silu(gate) * up out: the sums are exact, the comparison sees the epilogue alone (expf, the
    bf16 store) -- the bound of tests/test_gpu_linear_w4_ops.py::test_silu_gate_on_small_integers."""
    rs = np.random.RandomState(I + K + T)
    q, xi = pack(INT_CODE[rs.randint(0, 5, size=(2 * I, K))]), rs.randint(-2, 3, size=(T, K))
    e = (127 + rs.randint(-9, -5, size=(2 * I, K // 32))).astype(np.uint8)
    pre = xi.astype(np.float64) @ mx4_values(q, e).T.astype(np.float64)
    g, u = pre[:, :I], pre[:, I:]
    np.testing.assert_allclose(fa.op_linear_w4_tall(bf16(xi), q, e, epilogue=1), g / (1.0 + np.exp(-g)) * u, atol=1e-3, rtol=2 ** -8)
