"""k_gemv_w4.hip alone: the MXFP4 quantiser bit for bit against tests/test_w4_abi.py's restatement; fl_op_gemv_w4 against float64 numpy on 2^e * q."""
import numpy as np
import pytest

import synth
from test_gpu_w8_ops import fa  # noqa: F401  (the fixture)
from test_w4_abi import MIDS, mx4_values, quantize_mx4_ref

pytestmark = pytest.mark.gpu

# rows per row group is 4: N = 1, 5, 9, 33 are one more than a multiple of it, 3 and 7 end inside a group.  K: one block; two; one
# whole wave instruction (2048); one and a block; three instructions with a partial last (6112 = 191 blocks); 7 instructions (U = 1)
EDGE_SHAPES = [(1, 32), (3, 64), (5, 2048), (7, 2080), (33, 6112), (9, 14336)]
STEP_SHAPES = [(4096, 4096), (6144, 4096)]                 # Mistral-7B's o_proj and QKV: U = 2, one item per row group
GLU_SHAPES = [(40, 64), (352, 256), (14336, 4096)]


def _planted(K, bf16):
    """48 rows; block 0 of the first rows is planted, everything else is Gaussian under a row-dependent power of two."""
    rs = np.random.RandomState(K)
    w = (rs.standard_normal((48, K)) * 0.05).astype(np.float32) * np.ldexp(np.float32(1.0), np.arange(48) % 7 - 3)[:, None]
    tie_block = np.concatenate([[6.0], MIDS, -MIDS, np.zeros(17)]).astype(np.float32)
    w[0, :32] = 0.0                                        # a zero block
    w[1, :32] = np.clip(w[1, :32], -0.5, 0.5); w[1, 5] = -6.0 * 2.0 ** -3      # absmax exactly 6 * 2^e
    w[2, :32] = tie_block                                  # every midpoint in both signs, e = 0
    w[3, :32] = tie_block * np.float32(2.0 ** -5)          # and under another scale
    w[4, :32] = 1e-4 * rs.standard_normal(32); w[4, 17] = 3.0                   # one outlier, the rest near zero
    w[5, :32] = np.float32(2.0 ** -125) * rs.randint(-3, 4, size=32)            # absmax below 2^-120: the exponent floor
    return synth.bf16_bits_to_f32(synth.f32_to_bf16_bits(w)) if bf16 else w


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("K", [32, 4096])
def test_quantize_mx4_bit_for_bit(fa, K, bf16):
    w = _planted(K, bf16)
    q, e = fa.op_quantize_mx4(synth.f32_to_bf16_bits(w) if bf16 else w)
    qr, er = quantize_mx4_ref(w)
    assert er[0, 0] == 127 and er[1, 0] == 124 and er[2, 0] == 127 and er[3, 0] == 122 and er[5, 0] == 7, er[:6, 0]
    np.testing.assert_array_equal(e, er)
    np.testing.assert_array_equal(q, qr)


@pytest.mark.parametrize("e0", [-120, -14, 0, 5, 100])
def test_gemv_w4_every_code_at_every_place(fa, e0):
    """One-hot x: y == 2^e * value(code) for all 16 codes at both nibbles, each of a lane's four dwords, the second and the partial last instruction."""
    K = 2048 * 2 + 96
    codes = ((np.arange(16)[:, None] + 3 * np.arange(K)[None, :]) % 16).astype(np.uint8)
    q = codes[:, 0::2] | (codes[:, 1::2] << 4)
    e = np.tile((e0 + 127 + np.arange(K // 32) % 2).astype(np.uint8), (16, 1))
    want = mx4_values(q, e)
    for col in (0, 1, 9, 18, 27, 32 * 40 + 30, 2048 + 37, 4096 + 64 + 13):
        x = np.zeros(K, dtype=np.uint16)
        x[col] = 0x3F80                                    # 1.0
        np.testing.assert_array_equal(fa.op_gemv_w4(x, q, e), want[:, col], err_msg="column %d" % col)


def _int_case(rs, N, K, elo, ehi, xmax):
    q = rs.randint(0, 256, size=(N, K // 2)).astype(np.uint8)                  # every code, both signs
    e = (127 + rs.randint(elo, ehi + 1, size=(N, K // 32))).astype(np.uint8)
    x = rs.randint(-xmax, xmax + 1, size=K).astype(np.float32)
    return q, e, x, mx4_values(q, e).astype(np.float64) @ x.astype(np.float64)


@pytest.mark.parametrize("bias", [False, True], ids=["plain", "bias"])
@pytest.mark.parametrize("N,K", EDGE_SHAPES + STEP_SHAPES)
def test_gemv_w4_integer_exact(fa, N, K, bias):
    """Every code, block exponents in [-2, 2], integer x in [-3, 3]: terms are multiples of 2^-3 up to 72, fp32 sums exact in any order."""
    assert 72 * 8 * K < 2 ** 24
    rs = np.random.RandomState(N + 3 * K)
    q, e, x, pre = _int_case(rs, N, K, -2, 2, 3)
    b = rs.randint(-8, 9, size=N).astype(np.float32) if bias else None
    y = fa.op_gemv_w4(synth.f32_to_bf16_bits(x), q, e, bias=b)
    np.testing.assert_array_equal(y, (pre + b if bias else pre).astype(np.float32))


@pytest.mark.parametrize("N,K", EDGE_SHAPES + [(4096, 14336)])
def test_gemv_w4_random_operands(fa, N, K):
    """N(0, 0.05^2) weights through the restatement, N(0, 1) x in bf16: the bound of tests/test_gpu_w8_ops.py::test_gemv_w8_random_operands."""
    rs = np.random.RandomState(N + 3 * K)
    q, e = quantize_mx4_ref((rs.standard_normal((N, K)) * 0.05).astype(np.float32))
    xb = synth.f32_to_bf16_bits(rs.standard_normal(K).astype(np.float32))
    b = rs.standard_normal(N).astype(np.float32)
    ref = mx4_values(q, e).astype(np.float64) @ synth.bf16_bits_to_f32(xb).astype(np.float64) + b
    np.testing.assert_allclose(fa.op_gemv_w4(xb, q, e, bias=b), ref, atol=2e-5 * np.sqrt(K) + 1e-5, rtol=1e-5)


@pytest.mark.parametrize("I,K", GLU_SHAPES)
def test_gemv_w4_silu_gate_on_small_integers(fa, I, K):
    """gate | up rows in HF order; integer operands, exact sums: the epilogue alone, under the bound of test_gemv_w8_silu_gate_on_small_integers."""
    assert 6 * 2 * 2 ** 3 * K < 2 ** 24                    # terms: multiples of 2^-9, at most 6 * 2^-6 * 2
    rs = np.random.RandomState(I + K)
    q, e, x, pre = _int_case(rs, 2 * I, K, -8, -6, 2)
    y = fa.op_gemv_w4(synth.f32_to_bf16_bits(x), q, e, epilogue=1)
    np.testing.assert_allclose(y, pre[:I] / (1.0 + np.exp(-pre[:I])) * pre[I:], atol=1e-3, rtol=2 ** -8)


@pytest.mark.parametrize("K", [16, 48, 4100])
def test_gemv_w4_refuses_k_that_is_not_whole_blocks(fa, K):
    with pytest.raises(fa.FastLLMError) as err:
        fa.op_gemv_w4(np.zeros(K, dtype=np.uint16), np.zeros((4, K // 2), dtype=np.uint8), np.zeros((4, K // 32), dtype=np.uint8))
    assert err.value.code == -10
