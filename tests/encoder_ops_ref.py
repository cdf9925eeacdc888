"""Reference of the encoder's row kernels (k_encoder.hip: embedding sum + LayerNorm, residual add + LayerNorm, bias + GELU, pooling) for
tests/test_gpu_encoder_ops.py.  What the kernels do in fp32 in the one order there is -- the pre-norm sums, the slab + bias sums, the
column means -- is redone in numpy float32 and compared bit for bit; LayerNorm, GELU and the L2 normalisation are computed in float64 on
those exact fp32 values and compared within bounds that are DERIVED below (from the count of fp32 roundings), never measured on a
kernel.  tests/test_encoder_ops_ref.py checks the bounds on the CPU: a float32 restatement of the kernels stays inside them and planted
errors do not."""
import math

import numpy as np

import norm_ref
import rope_ref
import synth

U = 2.0 ** -24                     # unit roundoff of fp32

# ---- inputs -------------------------------------------------------------------------------------------------------------------------
# The rows of a LayerNorm case as (mean, std): zero-mean O(1) rows -- all the end-to-end tests ever see --, rows whose mean is 100 and
# 1000 standard deviations away (a one-pass E[x^2] - mean^2 variance cancels there), a row whose variance is below eps = 1e-5 and one
# whose variance is near it (the wrong eps shows there).  No constant rows: a zero-variance row divides rounding noise by sqrt(eps).
KINDS = ((0.0, 1.0), (100.0, 1.0), (1000.0, 1.0), (0.0, 1e-3), (3.0, 2.0 ** -6))
EPS = (1e-5, 1e-12)                # the layers' (a config's) and the embeddings' hard-wired one

LN_H = (8, 512, 520, 768, 1032)    # one lane active | every lane one chunk | lane 0 alone on a second trip | BERT-base | a third trip
LN_SHAPES = [(9, h) for h in LN_H] + [(T, 520) for T in (1, 4, 5)]          # (T, h); T around the 4 rows of a workgroup
EMBED_LENGTHS = {1: [1], 4: [1, 3], 5: [2, 3], 9: [1, 3, 2, 3]}             # the sequences of an embedding case of T rows
ACT_SHAPES = [(1, 8), (3, 24), (32, 64), (257, 8), (5, 1536)]               # (T, N): 1 chunk | cpr 3 | 256 chunks | 257 | MiniLM's I
POOL_H = (8, 256, 264, 576, 1032)  # threads beyond h | one trip | a partial second | MiniLM-like | a fifth trip of 8 threads
POOL_LENGTHS = ([1, 2, 17, 300], [1])


def row_kind(t):
    return t % len(KINDS)


def kind_rows(T, h, rs):
    """[T, h] float32: row t has the statistics of KINDS[t % 5]; rows 0..4 as written, later rows times norm_ref.row_scales' power of
    two (so that rows of one kind still differ by a factor)"""
    sc = norm_ref.row_scales(T)[:, 0].astype(np.float64)
    sc[:len(KINDS)] = 1.0
    k = np.arange(T) % len(KINDS)
    mean, std = np.array([KINDS[i][0] for i in k]), np.array([KINDS[i][1] for i in k])
    return ((mean[:, None] + std[:, None] * rs.standard_normal((T, h))) * sc[:, None]).astype(np.float32)


def _ln_params(h, rs):
    return rs.uniform(0.5, 1.5, size=h).astype(np.float32), (0.5 * rs.standard_normal(h)).astype(np.float32)


def _tab(a, dtype):
    """a float32 table as the library takes it (bf16 bits or float32) and the float32 values those are"""
    bits, vals = norm_ref.as_dtype(np.ascontiguousarray(a, dtype=np.float32), dtype)
    return bits, np.ascontiguousarray(vals, dtype=np.float32)


def embed_case(T, h, dtype, seed=0):
    """launch_encoder_embed_ln: distinct ids whose word rows are kind_rows (every other word row is N(0, 8^2): a wrong id is gross),
    distinct position rows N(0, 2^-14) -- small beside every kind but the fourth, and they keep a bf16-rounded row from being
    constant -- and a token-type row N(0, 0.5^2).  Tables in `dtype`."""
    rs = np.random.RandomState(1000 + 17 * T + h + seed)
    lengths = EMBED_LENGTHS[T]
    vocab, P = 2 * T + 7, max(lengths) + 3
    ids = rs.permutation(vocab)[:T].astype(np.uint32)
    word = (8.0 * rs.standard_normal((vocab, h))).astype(np.float32)
    word[ids] = kind_rows(T, h, rs)
    pos = (2.0 ** -7 * rs.standard_normal((P, h))).astype(np.float32)
    tt0 = (0.5 * rs.standard_normal(h)).astype(np.float32)
    w, b = _ln_params(h, rs)
    c = dict(T=T, h=h, dtype=dtype, lengths=lengths, ids=ids, w=w, b=b)
    for name, a in (("word", word), ("pos", pos), ("tt0", tt0)):
        c[name + "_bits"], c[name] = _tab(a, dtype)
    return c


def embed_prenorm(c, with_tt0):
    """(word[id] + pos[t - offsets[s]]) (+ tt0): fp32 adds of the widened values in the kernel's order"""
    p = np.concatenate([np.arange(n) for n in c["lengths"]])
    v = c["word"][c["ids"]] + c["pos"][p]
    if with_tt0:
        v = v + c["tt0"][None, :]
    assert v.dtype == np.float32
    return v


def slab_scales(n_slab, T):
    """slab s, row t times 2^((3 s + 5 t) % 7 - 3): 3 s mod 7 is distinct for s < 7, so in every row each slab has a scale of its own
    -- a slab read at the wrong stride, read twice or skipped moves the sum by a factor -- and neighbouring rows differ too"""
    s, t = np.arange(n_slab)[:, None], np.arange(T)[None, :]
    return (2.0 ** ((3 * s + 5 * t) % 7 - 3)).astype(np.float32)[:, :, None]


def slab_sum(slabs, bias):
    """slab 0 + slab 1 + ... (+ bias), float32, in slab order: the kernels' `d`"""
    d = np.array(slabs[0], dtype=np.float32, copy=True)
    for s in range(1, len(slabs)):
        d = d + slabs[s]
    if bias is not None:
        d = d + bias[None, :]
    assert d.dtype == np.float32
    return d


def add_ln_case(T, h, n_slab, with_bias, seed=0):
    """launch_encoder_add_ln: slabs N(0, 1) times slab_scales, bias N(0, 1) per column, and x = kind_rows - (slab sum), so that the
    pre-norm rows x + (slab sum) have the kinds' statistics (up to the rounding of that subtraction)"""
    rs = np.random.RandomState(2000 + 17 * T + h + 131 * n_slab + (7 if with_bias else 0) + seed)
    slabs = rs.standard_normal((n_slab, T, h)).astype(np.float32) * slab_scales(n_slab, T)
    bias = rs.standard_normal(h).astype(np.float32) if with_bias else None
    x = (kind_rows(T, h, rs) - slab_sum(slabs, bias)).astype(np.float32)
    w, b = _ln_params(h, rs)
    return dict(T=T, h=h, x=x, slabs=slabs, bias=bias, w=w, b=b)


def add_ln_prenorm(c):
    """x + (slab 0 + slab 1 + ... + bias): the slabs and the bias are summed first, then added to x"""
    v = c["x"] + slab_sum(c["slabs"], c["bias"])
    assert v.dtype == np.float32
    return v


def act_case(T, N, n_slab, with_bias, seed=0):
    """launch_encoder_bias_act: pre-activations on a grid over [-12, 12] (the first half of the elements) and N(0, 3^2) (the rest); the
    last element is 2.25, near where the tanh and the erf form are farthest apart, so that every case tells them apart.
    bias N(0, 1), distinct per column; slabs 1.. are N(0, 1) times slab_scales and slab 0 = target - (the others + bias)."""
    rs = np.random.RandomState(3000 + 17 * T + N + 131 * n_slab + (7 if with_bias else 0) + seed)
    n = T * N
    target = np.concatenate([np.linspace(-12.0, 12.0, n // 2), 3.0 * rs.standard_normal(n - n // 2)]).astype(np.float32).reshape(T, N)
    target[-1, -1] = 2.25
    slabs = rs.standard_normal((n_slab, T, N)).astype(np.float32) * slab_scales(n_slab, T)
    bias = rs.standard_normal(N).astype(np.float32) if with_bias else None
    rest = np.zeros((T, N), np.float32)
    for s in range(1, n_slab):
        rest = rest + slabs[s]
    if bias is not None:
        rest = rest + bias[None, :]
    slabs[0] = target - rest
    return dict(T=T, N=N, slabs=slabs, bias=bias)


def pool_case(lengths, h, seed=0):
    """launch_encoder_pool_l2: rows N(0, 1) + 0.25 (a mean that does not vanish) times norm_ref.row_scales"""
    T = int(sum(lengths))
    rs = np.random.RandomState(4000 + T + h + seed)
    return ((rs.standard_normal((T, h)) + 0.25).astype(np.float32) * norm_ref.row_scales(T)).astype(np.float32)


def pool_means(x, lengths):
    """the column means of each member, float32: adds in row order from +0, one divide by float32(len)"""
    out, r = [], 0
    for n in lengths:
        acc = np.zeros(x.shape[1], np.float32)
        for t in range(n):
            acc = acc + x[r + t]
        out.append(acc / np.float32(n))
        r += n
    out = np.stack(out)
    assert out.dtype == np.float32
    return out


# ---- LayerNorm ----------------------------------------------------------------------------------------------------------------------
def ln_ref(v, w, b, eps):
    """float64 LayerNorm of the exact fp32 pre-norm rows v [T, h] -> (o, mean, sd)"""
    v64 = v.astype(np.float64)
    mean = v64.mean(axis=1, keepdims=True)
    sd = np.sqrt(((v64 - mean) ** 2).mean(axis=1, keepdims=True) + eps)
    return (v64 - mean) / sd * w.astype(np.float64) + b.astype(np.float64), mean, sd


def ln_bound(v, w, b, eps):
    """(o, lim): the float64 LayerNorm and what ln_finish (k_encoder.hip) may differ from it by, per element, to first order in
    u = 2^-24:

        lim = u * ( |w| / sd * (n M + (n / 2 + 6) |v - mean|) + 2 |o| + |b| ),   n = 8 ceil(h / 512) + 7,   M = mean |v|

    * the fp32 mean: a lane adds its 8 ceil(h / 512) values one by one, the wave adds the 64 lanes in 6 shuffle steps, one divide:
      every value passes at most n roundings, each at most u times a partial sum that is at most sum |v|, so |mean' - mean| <= n u M.
      That error shifts every (v - mean) of the row alike: the first term.  (It enters the variance only at second order: the
      deviations sum to zero.)
    * (v - mean') rounds once; the variance is again a chain of at most n roundings on a sum of non-negative terms (fma: one rounding
      per term) plus two for each squared deviation, the + eps and the divide, and the square root halves its relative error and adds
      one: (n + 4) / 2 + 1; the divide by sd is one more.  1 + (n / 2 + 3) + 1 = n / 2 + 5, taken as n / 2 + 6: the second term.
    * `* w + b`: fused it rounds once, u |o|; unfused the product rounds at u |o - b| <= u (|o| + |b|) and the sum at u |o|.  Nothing
      in the build pins which one the compiler emits, so the bound takes the larger: 2 |o| + |b|."""
    T, h = v.shape
    o, mean, sd = ln_ref(v, w, b, eps)
    n = 8 * -(-h // 512) + 7
    v64 = v.astype(np.float64)
    M = np.abs(v64).mean(axis=1, keepdims=True)
    lim = U * (np.abs(w.astype(np.float64)) / sd * (n * M + (n / 2 + 6) * np.abs(v64 - mean)) + 2 * np.abs(o) + np.abs(b.astype(np.float64)))
    return o, lim


def wave_sum(p):
    """common.h's wave_sum on [T, 64] float32: v += shfl_xor(v, o) for o = 32, 16, ..., 1 (every lane ends with the same value)"""
    idx = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        p = p + p[:, idx ^ o]
    assert p.dtype == np.float32
    return p[:, 0]


def _fma32(a, b, c):
    """fmaf in float32: the product of two float32 is exact in float64; the sum then rounds to float64 and to float32 (a double
    rounding, which is good enough for a restatement that is compared within a bound, not bit for bit)"""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def ln_restate(v, w, b, eps, fused):
    """ln_finish in numpy float32 with the kernel's lane partition (lane l owns the chunks l, l + 64, ... of 8 columns), its lane
    chains, its butterfly and `* w + b` fused or not"""
    T, h = v.shape
    trips = -(-(h // 8) // 64)
    pad = np.zeros((T, trips * 512), np.float32)
    pad[:, :h] = v
    live = (np.arange(trips * 512) < h).reshape(trips, 64, 8)
    L = pad.reshape(T, trips, 64, 8)
    s = np.zeros((T, 64), np.float32)
    for t in range(trips):
        for j in range(8):
            s = s + L[:, t, :, j]                                   # (+ 0 where the lane has no chunk)
    mean = wave_sum(s) / np.float32(h)
    sq = np.zeros((T, 64), np.float32)
    for t in range(trips):
        for j in range(8):
            dl = np.where(live[t, :, j][None, :], L[:, t, :, j] - mean[:, None], np.float32(0))
            sq = _fma32(dl, dl, sq)
    sd = np.sqrt(wave_sum(sq) / np.float32(h) + np.float32(eps))
    q = (v - mean[:, None]) / sd[:, None]
    o = _fma32(q, np.broadcast_to(w, q.shape), np.broadcast_to(b, q.shape)) if fused else q * w[None, :] + b[None, :]
    assert mean.dtype == sd.dtype == q.dtype == o.dtype == np.float32
    return o


def ln_planted(v, w, b, eps, what):
    """LayerNorm as a subtly wrong kernel would compute it: "hm1" the unbiased variance (divisor h - 1), "onepass" the variance as
    E[x^2] - mean^2 with both moments in float32, "eps" the other eps of EPS"""
    v64, w64, b64 = v.astype(np.float64), w.astype(np.float64), b.astype(np.float64)
    h = v.shape[1]
    mean = v64.mean(axis=1, keepdims=True)
    var = ((v64 - mean) ** 2).mean(axis=1, keepdims=True)
    if what == "hm1":
        var = var * h / (h - 1.0)
    elif what == "onepass":
        m32 = v.sum(axis=1, keepdims=True, dtype=np.float32) / np.float32(h)
        q32 = (v * v).sum(axis=1, keepdims=True, dtype=np.float32) / np.float32(h)
        mean, var = m32.astype(np.float64), np.maximum((q32 - m32 * m32).astype(np.float64), 0.0)
    else:
        assert what == "eps"
        eps = EPS[1] if eps == EPS[0] else EPS[0]
    return (v64 - mean) / np.sqrt(var + eps) * w64 + b64


# ---- bias + GELU --------------------------------------------------------------------------------------------------------------------
_erf = np.vectorize(math.erf, otypes=[np.float64])


def gelu64(v, act):
    """float64 GELU of the exact fp32 pre-activations v (math.erf / np.tanh)"""
    v = v.astype(np.float64)
    if act == "gelu_erf":
        return 0.5 * v * (1.0 + _erf(v * math.sqrt(0.5)))
    assert act == "gelu_tanh"
    return 0.5 * v * (1.0 + np.tanh(math.sqrt(2.0 / math.pi) * v * (1.0 + 0.044715 * v * v)))


def gelu32(v, act):
    """enc_act in numpy float32: the kernel's constants (rounded to float32) and its order of operations"""
    one, half = np.float32(1.0), np.float32(0.5)
    if act == "gelu_erf":
        return half * v * (one + _erf((v * np.float32(0.7071067811865476)).astype(np.float64)).astype(np.float32))
    t = np.tanh(np.float32(0.7978845608028654) * v * (one + np.float32(0.044715) * v * v))
    assert t.dtype == np.float32
    return half * v * (one + t)


def gelu_bound(v, act, dtype):
    """(g, lim): the float64 GELU and what enc_act may differ from it by.

        fp32:  lim32 = u * (4 |g| + 16 |v|)
        bf16:  lim32 + max(half a bf16 ulp of g, lim32)

    * 16 |v|: a device erff of 4 ulp / tanhf of 2 ulp (the figures of the HIP math documentation; the argument's own two or three
      roundings move tanh and erf by less than that again where they are not flat) is at most 4 u at 1 + f ~ 1, the sum rounds once,
      and the result is multiplied by 0.5 |v|: about 3 u |v|, taken with margin.  It does not shrink with g, which is what the
      negative tail needs: there 1 + f cancels and g is far smaller than v.
    * 4 |g|: the two roundings of 0.5 * v * (...), with margin.
    * bf16: the fp32 value y (within lim32 of g) is rounded to nearest.  If y lies in g's binade or below, that costs at most half a
      bf16 ulp of g, 2^-8 * 2^floor(log2 |g|); if y has crossed the next power of two -- a bf16 value -- the rounded value is no
      farther from y than that power is, which is at most lim32.  (2^-9 |g| would be less than half an ulp for every g that is not
      just below a power of two: the correctly rounded reference itself misses it, tests/test_encoder_ops_ref.py.)"""
    g = gelu64(v, act)
    lim = U * (4 * np.abs(g) + 16 * np.abs(v.astype(np.float64)))
    if dtype == "bf16":
        lim = lim + np.maximum(rope_ref.half_ulp_bf16(g), lim)
    return g, lim


# ---- helpers ------------------------------------------------------------------------------------------------------------------------
def widen(a):
    """bf16 bits or float32 -> float64 values"""
    return rope_ref.widen(a)


def as_stored(a, dtype):
    """float32 values as a kernel stores them in `dtype`: RNE bf16 bits, or the float32 bits"""
    a = np.ascontiguousarray(a, dtype=np.float32)
    return synth.f32_to_bf16_bits(a) if dtype == "bf16" else a


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def worst(err, lim):
    """max err / lim over the elements (lim > 0 everywhere a test uses it)"""
    return float((np.abs(err) / np.maximum(lim, 1e-300)).max())
