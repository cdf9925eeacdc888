"""Reference of "residual add -> RMSNorm -> projection" for tests/test_gpu_norm_ops.py: everything the kernels do in fp32 is redone in
numpy float32 in the one rounding order there is (and compared bit for bit), everything else in float64."""
import numpy as np

import synth

EPS = 1e-5

# 1/rms, derived (not measured).  rmsnorm_add / the norm prologues: the longest fp32 chain of a sum of squares for h <= 8192 is
# 32 fmaf + 6 shuffle adds + 3 adds (41 roundings of 2^-24 on a sum of positives); 1/sqrt halves the relative error, plus a few ulp
# for sqrt, the divide and + eps.
INV_RTOL = 2e-6


def inv_parts_rtol(np_):
    """... from the residual epilogue's partial sums: 4 fmaf, 4 shuffle adds and np adds left to right; one missing or doubled slot
    of np moves the sum by about 1 / np >= 0.8 %."""
    return (np_ + 16) * 2.0 ** -24


def proj_tol(K, epi):
    """tests/test_gpu_ops.py's projection tolerances (the normalised activations are O(1)): (atol, rtol)"""
    return (2e-3, 2.0 ** -7) if epi else (2e-5 * np.sqrt(K) + 1e-5, 1e-5)


def row_scales(T):
    """Row t of every input with T > 1 is scaled by 2^((7 t) % 11 - 5): the period divides no tile height, so a row scale taken from
    a neighbouring row, a neighbouring tile or a clamped row moves the result by at least a factor of 2."""
    if T <= 1:
        return np.ones((max(T, 1), 1), np.float32)
    return (np.float32(2.0) ** ((7 * np.arange(T)) % 11 - 5)).astype(np.float32)[:, None]


def inputs(T, h, n_slab, seed):
    """x [T, h] and delta [n_slab, T, h] (None for n_slab 0): N(0, 1) times the row scale; w [h] uniform in [0.5, 1.5]"""
    rs = np.random.RandomState(seed)
    sc = row_scales(T)
    x = rs.standard_normal((T, h)).astype(np.float32) * sc
    delta = (rs.standard_normal((n_slab, T, h)).astype(np.float32) * sc[None]) if n_slab else None
    w = rs.uniform(0.5, 1.5, size=h).astype(np.float32)
    return x, delta, w


def weights(N, K, seed, bias=False):
    rs = np.random.RandomState(seed)
    W = (rs.standard_normal((N, K)) * 0.05).astype(np.float32)
    return W, (rs.standard_normal(N).astype(np.float32) if bias else None)


def residual(x, delta):
    """v = x + delta[0] + delta[1] + ... in float32, slab by slab in slab order: the one order every form sums them in"""
    v = np.array(x, dtype=np.float32, copy=True)
    if delta is None:
        return v
    for s in range(len(delta)):
        v = v + delta[s]
    return v


def xs_of(v, w, dtype):
    """xs = float32(v * w), rounded to bf16 (RNE, as the kernels' conversion) for dtype "bf16"; returned widened to float32"""
    xs = (v.astype(np.float32) * w.astype(np.float32)[None, :]).astype(np.float32)
    return synth.bf16_bits_to_f32(synth.f32_to_bf16_bits(xs)) if dtype == "bf16" else xs


def inv_rms(v, eps=EPS):
    v64 = v.astype(np.float64)
    return 1.0 / np.sqrt((v64 * v64).mean(axis=1) + eps)


def silu_gate(y):
    I = y.shape[1] // 2
    g, u = y[:, :I], y[:, I:]
    return g / (1.0 + np.exp(-g)) * u


def project(xs, inv, W, bias=None, epi=0):
    """y = inv[t] * (xs[t] . W^T) + bias, and silu(gate) * up for epilogue 1 (W rows gate | up), in float64 on the exact xs"""
    y = (xs.astype(np.float64) @ W.astype(np.float64).T) * np.asarray(inv, dtype=np.float64)[:, None]
    if bias is not None:
        y = y + bias.astype(np.float64)
    return silu_gate(y) if epi else y


def as_dtype(a, dtype):
    """a float32 matrix as the library takes it: bf16 bits (uint16) or float32; and the values those are"""
    if dtype == "bf16":
        bits = synth.f32_to_bf16_bits(a)
        return bits, synth.bf16_bits_to_f32(bits)
    return np.ascontiguousarray(a, dtype=np.float32), a
