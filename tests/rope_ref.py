"""Reference of "QKV projection -> RoPE -> KV append" for tests/test_gpu_rope_ops.py (numpy only).  The stand-alone kernels sum their
slabs, add the bias and rotate in fp32 in one rounding order -- redone here in numpy float32 and compared bit for bit; the fused forms
accumulate in their own order and are compared with a float64 rotation under the derived bound below."""
import numpy as np

import norm_ref
import synth

THETA = 10000.0


def tables(max_pos, d, theta=THETA):
    """cos / sin [max_pos, d / 2] float32 as build_rope (weights.hip) states them: inv_freq[j] = 1 / theta^(2j/d) in fp32, the angle an
    fp32 product, cosf / sinf.  The tests hand these tables to the ops: the kernels only index them."""
    j = np.arange(d // 2, dtype=np.float32)
    inv = (np.float32(1.0) / np.power(np.float32(theta), (np.float32(2.0) * j) / np.float32(d), dtype=np.float32)).astype(np.float32)
    ang = (np.arange(max_pos, dtype=np.float32)[:, None] * inv[None, :]).astype(np.float32)
    return np.cos(ang, dtype=np.float32), np.sin(ang, dtype=np.float32)


def sum_slabs(qkv, bias=None):
    """qkv [n_slab, rows, N] -> [rows, N]: slab 0 + slab 1 + ... in float32 in slab order, then + bias in float32"""
    qkv = np.asarray(qkv, dtype=np.float32)
    y = qkv[0].copy()
    for s in range(1, qkv.shape[0]):
        y = (y + qkv[s]).astype(np.float32)
    if bias is not None:
        y = (y + np.asarray(bias, dtype=np.float32)[None, :]).astype(np.float32)
    return y


def _split(y, H, Hkv, d):
    rows = y.shape[0]
    q, k, v = y[:, :H * d], y[:, H * d:(H + Hkv) * d], y[:, (H + Hkv) * d:]
    return q.reshape(rows, H, d), k.reshape(rows, Hkv, d), v.reshape(rows, Hkv, d)


def rotate_exact(x, cos, sin, pos, H, Hkv, d, dtype):
    """x [rows, (H + 2 Hkv) d] float32, pos [rows]: rotate-half on the q and k heads at cos / sin[pos] in float32 with separately rounded
    products -- ra = f32(f32(a c) - f32(b s)), rb = f32(f32(a s) + f32(b c)), what rope_rotate (common.h) computes -- and v as it is.
    Returns (q [rows, H d], k [rows, Hkv d], v [rows, Hkv d]): bf16 bits (uint16, RNE as the kernels convert) for dtype "bf16", else float32."""
    x = np.asarray(x, dtype=np.float32)
    half = d // 2
    c, s = np.asarray(cos, np.float32)[pos][:, None, :], np.asarray(sin, np.float32)[pos][:, None, :]
    out = []
    for part in _split(x, H, Hkv, d)[:2]:
        a, b = part[..., :half], part[..., half:]
        ra = ((a * c).astype(np.float32) - (b * s).astype(np.float32)).astype(np.float32)
        rb = ((a * s).astype(np.float32) + (b * c).astype(np.float32)).astype(np.float32)
        out.append(np.concatenate([ra, rb], axis=-1).reshape(x.shape[0], -1))
    out.append(np.ascontiguousarray(x[:, (H + Hkv) * d:]))
    return tuple(synth.f32_to_bf16_bits(o) if dtype == "bf16" else o for o in out)


def rotate64(y, cos, sin, pos, H, Hkv, d):
    """the same in float64 from a float64 projection y, the angles' cos / sin taken from the fp32 tables.  Returns (q, k, v) float64 and
    (mq, mk): max(|a|, |b|) of every rotated element's pair, which the bound needs"""
    y = np.asarray(y, dtype=np.float64)
    half = d // 2
    c, s = np.asarray(cos, np.float64)[pos][:, None, :], np.asarray(sin, np.float64)[pos][:, None, :]
    out, mags = [], []
    for part in _split(y, H, Hkv, d)[:2]:
        a, b = part[..., :half], part[..., half:]
        out.append(np.concatenate([a * c - b * s, a * s + b * c], axis=-1).reshape(y.shape[0], -1))
        m = np.maximum(np.abs(a), np.abs(b))
        mags.append(np.concatenate([m, m], axis=-1).reshape(y.shape[0], -1))
    out.append(np.ascontiguousarray(y[:, (H + Hkv) * d:]))
    return tuple(out), tuple(mags)


def half_ulp_bf16(r):
    """half a bf16 ulp of |r| (0 at r = 0).  bf16 keeps 8 significant bits (1 implicit + 7 stored), so in [2^e, 2^(e+1)) its values are
    2^(e-7) apart and round-to-nearest errs by up to 2^(e-8) = 2^-8 * 2^floor(log2 |r|): 1 + 2^-8 lies exactly between the neighbours
    1 and 1 + 2^-7.  (A figure of 2^-9 * 2^e would be a quarter ulp, which a correctly rounded value does not meet:
    tests/test_rope_ref.py::test_half_ulp_is_what_rounding_needs.)"""
    r = np.abs(np.asarray(r, dtype=np.float64))
    return np.where(r > 0, 2.0 ** -8 * 2.0 ** np.floor(np.log2(np.where(r > 0, r, 1.0))), 0.0)


def fused_bounds(y, cos, sin, pos, H, Hkv, d, K, dtype):
    """What a fused form may give for the float64 projection y, derived (not measured): its pre-rotation value differs from y by at most
    the projection tolerance (atol_p, rtol_p) = norm_ref.proj_tol(K, 0); the rotation mixes two such values with |c|, |s| <= 1; one
    rounding to the cache dtype follows.  Returns ((q, k, v) float64, (lim_q, lim_k, lim_v))."""
    atol, rtol = norm_ref.proj_tol(K, 0)
    (q, k, v), (mq, mk) = rotate64(y, cos, sin, pos, H, Hkv, d)
    lims = [2.0 * (atol + rtol * mq), 2.0 * (atol + rtol * mk), atol + rtol * np.abs(v)]
    if dtype == "bf16":
        lims = [l + half_ulp_bf16(r) for l, r in zip(lims, (q, k, v))]
    return (q, k, v), tuple(lims)


def widen(a):
    """bf16 bits or float32 -> float64 values"""
    a = np.asarray(a)
    return (synth.bf16_bits_to_f32(a) if a.dtype == np.uint16 else a).astype(np.float64)


def pattern(shape, dtype, seed):
    """A recognisable cache image: every element a finite value in [1, 2) from a hash of its flat index (bf16: 7 mantissa bits, fp32:
    23), as bf16 bits (uint16) or float32.  No kernel output looks like it by accident, and a neighbour's value differs."""
    n = int(np.prod(shape))
    h = (np.arange(n, dtype=np.uint64) * np.uint64(2654435761) + np.uint64(seed) * np.uint64(40503)) & np.uint64(0xffffffff)
    h = (h ^ (h >> np.uint64(15))) * np.uint64(2246822519) & np.uint64(0xffffffff)
    h = h ^ (h >> np.uint64(13))
    if dtype == "bf16":
        return (np.uint16(0x3f80) | (h & np.uint64(0x7f)).astype(np.uint16)).reshape(shape)
    return (np.uint32(0x3f800000) | (h & np.uint64(0x7fffff)).astype(np.uint32)).view(np.float32).reshape(shape)


def new_caches(layers, Hkv, sa, d, vt, dtype, seed):
    """(K [layers, Hkv, sa, d], V the same or transposed [layers, Hkv, d, sa]) filled with the pattern"""
    k = pattern((layers, Hkv, sa, d), dtype, seed)
    v = pattern((layers, Hkv, d, sa) if vt else (layers, Hkv, sa, d), dtype, seed + 1)
    return k, v


def place(cache_k, cache_v, k, v, slot, vt, layer):
    """the full cache images after rows k / v [rows, Hkv d] went to slots slot[r] of `layer`: K [L, Hkv, sa, d], V the same or (vt)
    transposed [L, Hkv, d, sa]; copies, the inputs stay as they are"""
    ck, cv = np.array(cache_k, copy=True), np.array(cache_v, copy=True)
    Hkv, d = ck.shape[1], ck.shape[3]
    k, v = np.asarray(k).reshape(-1, Hkv, d), np.asarray(v).reshape(-1, Hkv, d)
    for r, s in enumerate(np.asarray(slot).reshape(-1)):
        ck[layer, :, s, :] = k[r]
        if vt:
            cv[layer, :, :, s] = v[r]
        else:
            cv[layer, :, s, :] = v[r]
    return ck, cv


def appended_mask(cache_k, slot, vt, layer):
    """boolean images (K, V) that are True exactly at the appended slots of `layer`"""
    mk = np.zeros(cache_k.shape, dtype=bool)
    mk[layer][:, np.asarray(slot).reshape(-1), :] = True
    mv = np.ascontiguousarray(np.swapaxes(mk, 2, 3)) if vt else mk.copy()
    return mk, mv


def qkv_inputs(n_slab, rows, N, seed, bias):
    """qkv [n_slab, rows, N] for the stand-alone kernels: N(0, 1) times norm_ref.row_scales -- a row taken from a neighbour is off by a
    factor of 2 or more -- and a bias [N] or None"""
    rs = np.random.RandomState(seed)
    qkv = rs.standard_normal((n_slab, rows, N)).astype(np.float32) * norm_ref.row_scales(rows)[None]
    return qkv, (rs.standard_normal(N).astype(np.float32) if bias else None)


def fused_inputs(T, K, H, Hkv, d, n_slab, bias, dtype, seed):
    """the inputs of a fused form (norm_ref's) and their float64 projection y [T, (H + 2 Hkv) d] on the exact xs and 1/rms"""
    x, delta, w = norm_ref.inputs(T, K, n_slab, seed)
    W, b = norm_ref.weights((H + 2 * Hkv) * d, K, seed + 1, bias)
    Wd, Wv = norm_ref.as_dtype(W, dtype)
    v = norm_ref.residual(x, delta)
    xs, inv = norm_ref.xs_of(v, w, dtype), norm_ref.inv_rms(v)
    return dict(x=x, delta=delta, w=w, Wd=Wd, Wv=Wv, b=b, v=v, xs=xs, inv=inv, y=norm_ref.project(xs, inv, Wv, b))
