"""The 17-64-row FP8 weight stream (k_gemm_rows64_w8.hip) alone, through fl_op_linear_w8_wide, against numpy: bit for bit where fp32
sums are exact, fp64 numpy on s * q otherwise.  Bounds and helpers are those of tests/test_gpu_linear_w8_ops.py."""
import numpy as np
import pytest

import synth
from test_w8_abi import dequantize, e4m3_to_f32, quantize_rows_ref

pytestmark = pytest.mark.gpu
UNSUPPORTED = -10

# one partial row group; a partial last 64-column block and an odd group count; several x blocks; K slices
SHAPES = [(3, 64), (33, 1040), (40, 4096 + 512), (129, 14336 + 16)]
CASES = [(T, N, K) for T in (17, 33, 48, 64) for N, K in SHAPES] + [(64, 6144, 4096)]          # ... and Mistral-7B's QKV
TABLE = e4m3_to_f32(np.arange(256, dtype=np.uint8))
CODE_OF = np.array([np.flatnonzero(TABLE == v)[0] for v in range(-3, 4)], dtype=np.uint8)     # integers -3..3 as e4m3 codes


@pytest.fixture(scope="module")
def fa():
    import fastllm_amd
    assert fastllm_amd.device_count() >= 1
    return fastllm_amd


def bf16(a):
    return synth.f32_to_bf16_bits(np.asarray(a, dtype=np.float32))


@pytest.mark.parametrize("T,N,K", CASES)
def test_bit_exact_on_small_integers(fa, T, N, K):
    """Weights and x integers in -3..3, s and the row scales powers of two: every partial sum is an integer below 2^24, so fp32
    accumulation is exact in any order -- over lanes, MFMA passes, x blocks and K slabs -- and the result equals numpy bit for bit."""
    rs = np.random.RandomState(T * 131 + N * 7 + K)
    wi, xi = rs.randint(-3, 4, size=(N, K)), rs.randint(-3, 4, size=(T, K))
    s = np.ldexp(np.float32(1.0), rs.randint(-6, 7, size=N)).astype(np.float32)
    r = np.ldexp(np.float32(1.0), rs.randint(-3, 4, size=T)).astype(np.float32)
    assert K * 9 < 2 ** 24
    if K == 14336 + 16:
        assert fa.op_linear_w8_wide_plan(T, N, K) > 1
    ref = (xi.astype(np.float64) @ wi.T.astype(np.float64)) * s[None, :] * r[:, None]
    y = fa.op_linear_w8_wide(bf16(xi), CODE_OF[wi + 3], s, row_scale=r)
    np.testing.assert_array_equal(y, ref.astype(np.float32))


@pytest.mark.parametrize("row", [0, 16, 32])
@pytest.mark.parametrize("col", [0, 9, 17, 63, 1039])
def test_converts_every_code_exactly(fa, col, row):
    """All 254 finite e4m3fn codes against a one-hot x (both byte halves of a lane's load, both MFMAs of a step, the partial last
    block; the first row of the first and second token tile and the last row of 33): y = s * value(code) exactly in the hot row,
    exactly 0 in the others."""
    codes = np.array([c for c in range(256) if (c & 0x7F) != 0x7F], dtype=np.uint8)
    N, K, T = len(codes), 1040, 33
    q, x = np.zeros((N, K), dtype=np.uint8), np.zeros((T, K), dtype=np.float32)
    q[:, col], x[row, col] = codes, 1.0
    want = np.zeros((T, N), dtype=np.float32)
    want[row] = e4m3_to_f32(codes) * np.float32(0.25)
    np.testing.assert_array_equal(fa.op_linear_w8_wide(bf16(x), q, np.full(N, 0.25, dtype=np.float32)), want)


@pytest.mark.parametrize("T,N,K", CASES)
def test_random_operands(fa, T, N, K):
    """Random weights through the quantiser's restatement, N(0,1) x and row scales, against fp64 numpy on s * q."""
    rs = np.random.RandomState(N + 3 * K + T)
    q, s = quantize_rows_ref((rs.standard_normal((N, K)) * 0.05).astype(np.float32))
    xb, r = bf16(rs.standard_normal((T, K))), rs.standard_normal(T).astype(np.float32)
    ref = (synth.bf16_bits_to_f32(xb).astype(np.float64) @ dequantize(q, s).astype(np.float64).T) * r[:, None].astype(np.float64)
    y = fa.op_linear_w8_wide(xb, q, s, row_scale=r)
    np.testing.assert_allclose(y, ref, atol=2e-5 * np.sqrt(K) + 1e-5, rtol=1e-5)


@pytest.mark.parametrize("T", [17, 64])
@pytest.mark.parametrize("I,K", [(40, 64), (24, 1040), (352, 256)])
def test_silu_gate_on_small_integers(fa, I, K, T):
    """gate | up rows in HF order in, silu(gate) * up out: the sums are exact, the comparison sees the epilogue alone (expf, the
    bf16 store)."""
    rs = np.random.RandomState(I + K + T)
    wi, xi = rs.randint(-2, 3, size=(2 * I, K)), rs.randint(-2, 3, size=(T, K))
    s = np.ldexp(np.float32(1.0), rs.randint(-9, -5, size=2 * I)).astype(np.float32)
    pre = (xi.astype(np.float64) @ wi.T.astype(np.float64)) * s[None, :]
    g, u = pre[:, :I], pre[:, I:]
    y = fa.op_linear_w8_wide(bf16(xi), CODE_OF[wi + 3], s, epilogue=1)
    np.testing.assert_allclose(y, g / (1.0 + np.exp(-g)) * u, atol=1e-3, rtol=2 ** -8)


@pytest.mark.parametrize("T,K", [(16, 64), (65, 64), (17, 72)])
def test_refusals(fa, T, K):
    with pytest.raises(fa.FastLLMError) as e:
        fa.op_linear_w8_wide(np.zeros((T, K), dtype=np.uint16), np.zeros((4, K), dtype=np.uint8), np.ones(4, dtype=np.float32))
    assert e.value.code == UNSUPPORTED
