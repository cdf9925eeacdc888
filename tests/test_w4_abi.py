"""The MXFP4 weight mode (FL_WEIGHTS_MXFP4) without a GPU: the refusals that need no device, and the yardstick of the GPU tests --
a numpy restatement of the format (the header's fl_weight_format states it) with its own checks:
    W'[n,k] = 2^e[n, k/32] * q[n,k],   e the smallest integer with absmax(block) / 2^e <= 6, at least -120 (zero block: e = 0),
    q = RNE_e2m1(W / 2^e), ties to the code whose mantissa bit is 0; byte j = element 2j (low nibble) | element 2j + 1; scale byte e + 127."""
import ctypes as C

import numpy as np
import pytest

import synth
from test_w8_abi import PROJECTIONS, L, Options, _create  # noqa: F401  (L: the library fixture)

GRID = np.array([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0], dtype=np.float32)
MIDS = np.array([0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0], dtype=np.float32)


def quantize_mx4_ref(w):
    """w float32 [N,K] -> (q uint8 [N,K/2], e uint8 [N,K/32])."""
    w = np.ascontiguousarray(w, dtype=np.float32)
    N, K = w.shape
    b = np.abs(w).reshape(N, K // 32, 32)
    amax = b.max(axis=2)
    m, x = np.frexp(amax)                                  # amax = m * 2^x, m in [0.5, 1); 6 = 0.75 * 2^3
    e = np.where(m <= 0.75, x - 3, x - 2)
    e = np.where(amax == 0, 0, np.maximum(e, -120)).astype(np.int32)
    v = (b * np.ldexp(np.float32(1.0), -e)[:, :, None]).reshape(N, K)          # exact: a power of two; <= 6
    code = np.searchsorted(MIDS, v, side="left").astype(np.uint8)              # a midpoint lands on the code below it ...
    code += np.isin(v, MIDS) & (code % 2 == 1)                                 # ... and moves up where that code's mantissa bit is 1
    code |= np.signbit(w).astype(np.uint8) << 3
    return code[:, 0::2] | (code[:, 1::2] << 4), (e + 127).astype(np.uint8)


def mx4_values(q, e):
    """(q [N,K/2], e [N,K/32]) -> float32 [N,K] = 2^e * q."""
    N, K = q.shape[0], 2 * q.shape[1]
    c = np.empty((N, K), dtype=np.uint8)
    c[:, 0::2], c[:, 1::2] = q & 15, q >> 4
    v = np.where(c & 8, -GRID[c & 7], GRID[c & 7])
    return v * np.repeat(np.ldexp(np.float32(1.0), e.astype(np.int32) - 127), 32, axis=1)


def mx4_image_weights(w):
    """synth weights (bf16 bits) -> the same with every projection matrix replaced by the bf16 bits of W' (blocks run along K: HF row order is fine)."""
    out = dict(w)
    for name in [n for n in w if n.endswith(PROJECTIONS)]:
        wp = mx4_values(*quantize_mx4_ref(synth.bf16_bits_to_f32(w[name])))
        out[name] = synth.f32_to_bf16_bits(wp)
        assert np.array_equal(synth.bf16_bits_to_f32(out[name]), wp), name      # 2^e * q is exact in bf16
    return out


def _block(vals):
    return np.pad(np.asarray(vals, dtype=np.float32), (0, 32 - len(vals)))[None]


@pytest.mark.parametrize("scale", [1.0, 2.0 ** -9, 2.0 ** 40])
def test_midpoints_round_to_the_even_code_in_both_signs(scale):
    mids, want = [0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0], [0.0, 1.0, 1.0, 2.0, 2.0, 4.0, 4.0]
    w = _block([6.0] + mids + [-m for m in mids]) * np.float32(scale)
    q, e = quantize_mx4_ref(w)
    assert 2.0 ** (int(e[0, 0]) - 127) == scale
    got = mx4_values(q, e)[0, :15] / np.float32(scale)
    assert list(got) == [6.0] + want + [-v for v in want], got
    assert np.array_equal(np.signbit(got[8:]), np.ones(7, dtype=bool))          # -0.25 keeps its sign: code 8


@pytest.mark.parametrize("x", [-7, 0, 11])
def test_scale_at_the_two_ends_of_its_range_and_a_zero_block(x):
    for top, code in ((6.0, 7), (4.0, 6)):                                      # absmax exactly 6 * 2^x and exactly 4 * 2^x: e = x, no saturation
        q, e = quantize_mx4_ref(_block([np.ldexp(top, x), np.ldexp(-0.5, x)]))
        assert e[0, 0] == x + 127 and q[0, 0] == (code | 9 << 4), (top, q[0, 0], e[0, 0])
    q, e = quantize_mx4_ref(np.zeros((1, 32), dtype=np.float32))
    assert e[0, 0] == 127 and not q.any()
    q, e = quantize_mx4_ref(_block([2.0 ** -125, -(2.0 ** -123)]))              # below the exponent floor: e stays -120, everything rounds to zero
    assert e[0, 0] == 7 and q[0, 0] == 0x80 and not q[0, 1:].any()


@pytest.mark.parametrize("e", [-120, 0, 126])
def test_products_survive_a_bf16_round_trip(e):
    codes = np.arange(16, dtype=np.uint8)
    if e == 126:
        codes = codes[(codes & 7) < 6]                     # 4 * 2^126 and 6 * 2^126 lie above bf16's largest finite value: e = 126 comes with q <= 3 only
    q = np.pad(codes, (0, 16 - len(codes)))[None]          # high nibbles zero
    v = mx4_values(q, np.full((1, 1), e + 127, dtype=np.uint8))
    assert np.isfinite(v).all() and np.array_equal(synth.bf16_bits_to_f32(synth.f32_to_bf16_bits(v)), v)
    assert np.array_equal(np.abs(v[0, 0:2 * len(codes):2]), GRID[codes & 7] * np.float32(2.0) ** e)


def test_refusals_come_before_the_device_probe(L):
    import fastllm_amd.binding as B
    assert B.WEIGHTS_MXFP4 == 2 and B.DECODE_WEIGHTS["mxfp4"] == 2
    for (rc, msg), word in ((_create(L, B.F32, 2), "BF16"), (_create(L, B.BF16, 2, tp=2), "tensor parallelism")):
        assert rc == -10 and "FL_WEIGHTS_MXFP4" in msg and word in msg, (rc, msg)
    cfg = B.make_config(dict(synth.CONFIGS["llama_a"], hidden_size=48))         # a multiple of 16, not of 32
    o, h = Options(C.sizeof(Options), 2), C.c_void_p()
    rc = L.fl_model_create_opts(C.byref(cfg), None, 0, B.BF16, None, C.cast(C.byref(o), C.POINTER(B.FlModelOptions)), C.byref(h))
    assert rc == -10 and "hidden_size" in L.fl_last_error().decode() and "multiple of 32" in L.fl_last_error().decode()
    rc, _ = _create(L, B.BF16, 2)
    assert rc in (-9, -2), rc                              # a good request gets as far as the device probe (-9) or the tensors (-2)
