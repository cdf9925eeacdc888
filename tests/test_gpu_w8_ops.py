"""The FP8 (e4m3fn + power-of-two row scale) quantiser and decode weight stream alone, through their unit-test hooks
(fl_op_quantize_rows, fl_op_gemv_w8), against the CPU restatement of tests/test_w8_abi.py and fp64 numpy."""
import numpy as np
import pytest

import synth
from test_w8_abi import dequantize, e4m3_to_f32, quantize_rows_ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fa():
    import fastllm_amd
    assert fastllm_amd.device_count() >= 1
    return fastllm_amd


# ---- quantiser: bit for bit (the division is by a power of two, the rounding is RNE in both) ------------------------------------
def _quantiser_rows(K, seed):
    rs = np.random.RandomState(seed)
    w = (rs.standard_normal((48, K)) * 0.02).astype(np.float32)
    w[3] = 0.0                                                             # zero row: s = 1, q = 0
    w[4] *= np.float32(448.0 * 2.0 ** -9) / np.abs(w[4]).max()             # absmax exactly 448 * 2^e
    w[4, np.abs(w[4]).argmax()] = np.float32(448.0 * 2.0 ** -9)
    # values that land in the e4m3 subnormal range (below 2^-6 after scaling) and on its rounding boundaries
    w[5] = 0.0
    w[5, 0] = 256.0                                                        # s = 1
    w[5, 1:17] = np.ldexp(np.float32(1.0), -np.arange(4, 20)).astype(np.float32)
    w[5, 17:33] = -3.0 * np.ldexp(np.float32(1.0), -np.arange(4, 20)).astype(np.float32)
    # ties: exactly between two e4m3 numbers at every binade (mantissa x.xxx1 in binary), both signs
    w[6] = 0.0
    w[6, 0] = 448.0
    m = (np.arange(8, 16) * 2 + 1).astype(np.float32) / 16.0               # 17/16 ... 31/16
    k = 1
    for ex in range(-6, 8):
        w[6, k:k + 8] = m * np.float32(2.0) ** ex
        w[6, k + 8:k + 16] = -m * np.float32(2.0) ** ex
        k += 16
        if k + 16 > K:
            break
    w[7] = w[6] * np.float32(2.0 ** -20)                                   # the same ties under another scale
    w[8, 0] = 3.0                                                          # an outlier: the rest of the row is mostly subnormal / zero
    return w


@pytest.mark.parametrize("K", [64, 4096, 14336])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_quantize_rows_equals_the_cpu_restatement_bit_for_bit(fa, K, dtype):
    w = _quantiser_rows(K, K)
    if dtype == "bf16":
        bits = synth.f32_to_bf16_bits(w)
        w = synth.bf16_bits_to_f32(bits)
        q, s = fa.op_quantize_rows(bits)
    else:
        q, s = fa.op_quantize_rows(w)
    qr, sr = quantize_rows_ref(w)
    assert np.array_equal(s, sr), (s[:10], sr[:10])
    bad = np.argwhere(q != qr)
    assert bad.size == 0, [(int(r), int(c), float(w[r, c]), int(q[r, c]), int(qr[r, c])) for r, c in bad[:8]]
    assert not ((q & 0x7F) == 0x7F).any()


# ---- the kernel ---------------------------------------------------------------------------------------------------------------
def _e4m3_codes_of(values):
    """float32 values exactly representable in e4m3 -> their codes"""
    import torch
    q = torch.from_numpy(np.ascontiguousarray(values, dtype=np.float32)).to(torch.float8_e4m3fn)
    assert np.array_equal(q.to(torch.float32).numpy(), values)
    return q.view(torch.uint8).numpy()


# every (N, K) the fused decode step of TinyLlama-1.1B, Mistral-7B and Qwen2-7B launches with the plain epilogue (QKV without its RoPE:
# the model tests cover that epilogue), and the edges: N not a multiple of the rows per pass (2), K = 64 (less than one wave
# instruction), K not a multiple of 16 x 64 elements (a partial last wave instruction, after 0 .. 3 full ones)
STEP_SHAPES = [(2560, 2048), (2048, 2048), (2048, 5632), (32000, 2048),                    # TinyLlama: qkv, o, down, lm_head
               (6144, 4096), (4096, 4096), (4096, 14336), (32000, 4096),                   # Mistral-7B
               (4608, 3584), (3584, 3584), (3584, 18944), (152064, 3584)]                  # Qwen2-7B
EDGE_SHAPES = [(1, 64), (3, 64), (33, 1040), (301, 16), (64, 1024 + 16), (7, 2048 + 48), (40, 3072 + 1008), (5, 4096 + 512), (129, 14336 + 16)]
GLU_SHAPES = [(5632, 2048), (14336, 4096), (18944, 3584), (40, 64), (352, 256), (24, 1040)]            # (I, K)


BLOCK = 8192                                               # rows per block of the CPU side (Qwen2-7B's lm_head is 545 M weights)


def _int_case(rs, N, K, lo, hi):
    """integer weights in [lo, hi] as e4m3 codes, integer x, and the exact sums q . x (float64)"""
    lut = _e4m3_codes_of(np.arange(lo, hi + 1).astype(np.float32))
    x = rs.randint(lo, hi + 1, size=K).astype(np.float32)
    q = np.empty((N, K), dtype=np.uint8)
    pre = np.empty(N, dtype=np.float64)
    for r0 in range(0, N, BLOCK):
        wi = rs.randint(lo, hi + 1, size=(min(BLOCK, N - r0), K))
        q[r0:r0 + BLOCK] = lut[wi - lo]
        pre[r0:r0 + BLOCK] = wi.astype(np.float64) @ x.astype(np.float64)
    return q, x, pre


def _rand_case(rs, N, K):
    """N(0, 0.05^2) weights through the restatement, N(0, 1) x in bf16, and s * q . x in float64"""
    xb = synth.f32_to_bf16_bits(rs.standard_normal(K).astype(np.float32))
    x64 = synth.bf16_bits_to_f32(xb).astype(np.float64)
    q, s, pre = np.empty((N, K), dtype=np.uint8), np.empty(N, dtype=np.float32), np.empty(N, dtype=np.float64)
    for r0 in range(0, N, BLOCK):
        w = (rs.standard_normal((min(BLOCK, N - r0), K)) * 0.05).astype(np.float32)
        q[r0:r0 + BLOCK], s[r0:r0 + BLOCK] = quantize_rows_ref(w)
        pre[r0:r0 + BLOCK] = dequantize(q[r0:r0 + BLOCK], s[r0:r0 + BLOCK]).astype(np.float64) @ x64
    return q, s, xb, pre


@pytest.mark.parametrize("N,K", STEP_SHAPES + EDGE_SHAPES)
def test_gemv_w8_bit_exact_on_small_integers(fa, N, K):
    """q small integers (exact in e4m3), x small integers, s powers of two: every product and partial sum is an integer below 2^24,
    so fp32 accumulation is exact in any order and the result equals numpy bit for bit."""
    rs = np.random.RandomState(N * 7 + K)
    q, x, pre = _int_case(rs, N, K, -3, 3)
    s = np.ldexp(np.float32(1.0), rs.randint(-6, 7, size=N)).astype(np.float32)
    assert K * 9 < 2 ** 24
    y = fa.op_gemv_w8(synth.f32_to_bf16_bits(x), q, s)
    ref = pre * s
    np.testing.assert_array_equal(y, ref.astype(np.float32))
    b = rs.randint(-5, 6, size=N).astype(np.float32)
    yb = fa.op_gemv_w8(synth.f32_to_bf16_bits(x), q, s, bias=b)
    np.testing.assert_array_equal(yb, (ref + b).astype(np.float32))


def test_gemv_w8_converts_every_code_exactly(fa):
    """All 254 finite e4m3fn codes (subnormals included) against a one-hot x: y = s * value(code), exactly."""
    codes = np.array([c for c in range(256) if (c & 0x7F) != 0x7F], dtype=np.uint8)
    N, K = len(codes), 1024 + 64
    for col in (0, 5, 17, 1023, 1087):                     # both byte pairs of a word, both x halves of a chunk, the partial last instruction
        q = np.zeros((N, K), dtype=np.uint8)
        q[:, col] = codes
        x = np.zeros(K, dtype=np.float32)
        x[col] = 1.0
        s = np.full(N, 0.25, dtype=np.float32)
        y = fa.op_gemv_w8(synth.f32_to_bf16_bits(x), q, s)
        np.testing.assert_array_equal(y, e4m3_to_f32(codes) * np.float32(0.25))


@pytest.mark.parametrize("I,K", GLU_SHAPES)
def test_gemv_w8_silu_gate_on_small_integers(fa, I, K):
    """gate/up rows in HF order in (the hook interleaves them as the model does), silu(gate) * up out.  Integer operands: the sums in
    front of the epilogue are exact, so the comparison with the same formula in fp64 sees the epilogue alone (expf, the bf16 store):
    the bound tests/test_gpu_ops.py::test_linear_silu_gate gives bf16."""
    rs = np.random.RandomState(I + K)
    q, x, pre = _int_case(rs, 2 * I, K, -2, 2)
    s = np.ldexp(np.float32(1.0), rs.randint(-9, -5, size=2 * I)).astype(np.float32)
    y = fa.op_gemv_w8(synth.f32_to_bf16_bits(x), q, s, epilogue=1)
    pre = pre * s
    g, u = pre[:I], pre[I:]
    ref = g / (1.0 + np.exp(-g)) * u
    np.testing.assert_allclose(y, ref, atol=1e-3, rtol=2 ** -8)


@pytest.mark.parametrize("N,K", [sh for sh in STEP_SHAPES if sh[0] < 100000] + EDGE_SHAPES)
def test_gemv_w8_random_operands(fa, N, K):
    """Random weights through the quantiser's restatement, random x: against fp64 numpy on s * q, the bound
    tests/test_gpu_ops.py::test_linear_plain gives the bf16 kernels on operands of this size.  (Qwen2-7B's lm_head, 545 M weights,
    is in the integer-exact test only: drawing and quantising that many Gaussians on the CPU takes minutes.)"""
    rs = np.random.RandomState(N + 3 * K)
    q, s, xb, pre = _rand_case(rs, N, K)
    b = rs.standard_normal(N).astype(np.float32)
    y = fa.op_gemv_w8(xb, q, s, bias=b)
    np.testing.assert_allclose(y, pre + b, atol=2e-5 * np.sqrt(K) + 1e-5, rtol=1e-5)


@pytest.mark.parametrize("I,K", GLU_SHAPES)
def test_gemv_w8_silu_gate_random_operands(fa, I, K):
    rs = np.random.RandomState(2 * I + K)
    q, s, xb, pre = _rand_case(rs, 2 * I, K)
    y = fa.op_gemv_w8(xb, q, s, epilogue=1)
    g, u = pre[:I], pre[I:]
    np.testing.assert_allclose(y, g / (1.0 + np.exp(-g)) * u, atol=1e-3, rtol=2 ** -8)


@pytest.mark.parametrize("K", [8, 24, 1032, 4100])
def test_gemv_w8_refuses_k_that_is_not_a_multiple_of_16(fa, K):
    """A lane of the stream loads 16 weights: other K are refused (FL_ERR_UNSUPPORTED), here and -- through hidden_size -- at
    fl_model_create_opts (tests/test_w8_abi.py)."""
    with pytest.raises(fa.FastLLMError) as e:
        fa.op_gemv_w8(np.zeros(K, dtype=np.uint16), np.zeros((4, K), dtype=np.uint8), np.ones(4, dtype=np.float32))
    assert e.value.code == -10
