"""Reference, emulation, error bound and cases for attn_oproj_rep_kernel (k_attn_rep.hip), the decode attention that every workgroup
of the o_proj launch redoes for itself on short caches.  numpy only; shared by test_attn_rep_ref.py (CPU) and
test_gpu_attn_rep_ops.py (the kernel through fl_op_attn_oproj_rep).

The kernel, as far as its arithmetic goes (re-read in k_attn_rep.hip and attn_mfma.h):
  * wave w of the 8 attends for kv head w // nslice (its G = H / Hkv query heads in the MFMA columns) over the 32-key tiles
    t = w % nslice (mod nslice), nslice = 8 / Hkv, in ascending order (the bursts of TB tiles only group the loads);
  * attn_tile: fp32 scores (bf16 x bf16 products are exact, fp32 accumulation) times scale; keys >= S masked to -inf; running max
    m, alpha = __expf(m_old - m_new), p = __expf(score - m_new); l = l * alpha + sum(p) from the UNROUNDED p; P rounded to bf16
    (RNE) for the numerator only, O = O * alpha + P . V with fp32 accumulation;
  * the slices of a head meet in LDS in slice order: M = max m_z, weight __expf(m_z - M) (0 for a slice that owns no key),
    L = sum l_z w_z, O = sum O_z w_z, x = bf16(O * (1 / L)) (RNE): the second bf16 rounding;
  * out[n] = sum_k W[n, k] x[k]: exact bf16 products accumulated in fp32 by v_dot2c_f32_bf16 (two products per instruction, 8 K / 512
    of them per lane), then a 6-step wave reduce.

Error bound (`bound`), derived, worst case, per element k of x and then per output row n:
  A_k = sum_j p_j |v_jk| (p the exact softmax weights).
  E_k = 2^-9 A_k                      P rounded to bf16: every weight moves by at most 2^-9 of itself, l does not
      + 2^-9 (|x_k| + 2^-9 A_k)       x rounded to bf16: half an ulp of the value that is rounded
      + f                             the fp32 term of attn_cases.f32_bound: 10 e32 + (1.4427 gmax + 2) 2^-23 max|v|
      + (tps + 3) 2^-24 A_k           "rescale chain": one fp32 rounding per alpha rescale of O (tps = tiles per slice), one for the
                                      merge weight, one for 1 / L and one for the product with it -- the rounding point the code
                                      shows beyond the issue's list; ~1e-6 of A
  B_n = sum_k |W_nk| E_k + (K / 2 + 8) 2^-24 sum_k |W_nk| (|x_k| + E_k)
                                      the second part: the accumulation in the dot instructions and the wave reduce, on the x the
                                      kernel holds (at most |x_k| + E_k)
No free factor.  The exact cases below are what catches an indexing error; this bound is what a rounding point nobody wrote down
would break.

Exact cases.  attn_cases.decode_selectors gives x = rows of V bit for bit (decoys in the stale tail and in the next kv head, 3e4
behind the rows).  Two exact W_o go with it: a signed selection matrix (row n has the one entry +-2^e, e in -3..3, at column
(n + off) % K: out[n] = +-2^e x[col] exactly, and every column is picked when N >= K), and small integers (W in -2..2, V integers
in -16..16: every partial sum is an integer below 2^24, exact in fp32 in any order)."""
import numpy as np

import attn_cases as ac
from test_gpu_attention_ops import reference as attn_reference

R_NW = 8
STALE = 3e4
LAYOUTS = [(8, 8), (4, 1), (6, 2), (12, 4), (5, 1), (8, 1), (16, 2), (32, 4)]      # (H, Hkv): G = 1, 4, 3, 3, 5, 8, 8, 8; nslice 1, 8, 4, 2, 8, 8, 4, 2
LARGE_N = {64: [(4, 1), (32, 4)], 128: [(4, 1), (16, 2)]}                         # GMAX 4 and 8 at each head size; K = 256 / 2048, 512 / 2048
MISTAKES = ("drop_last_key", "drop_slice", "kv_head", "row", "no_mask")


def tb(d):
    return 4 if d == 64 else 2


def nslice(Hkv):
    return R_NW // Hkv


def rpw(N):
    return 2 if N > 256 * R_NW else 1


def layouts(d):
    return [(H, Hkv) for H, Hkv in LAYOUTS if H * d <= 2048]


def n_list(d, H, Hkv):
    K = H * d
    return [1, 7, 9, K] + ([2048, 2049, 2048 + 17, 4096] if (H, Hkv) in LARGE_N[d] else [])


def model_max_sa(Hkv, d):
    """the largest cache allocation (a multiple of 32 rows) the model's rule takes: Hkv sa d <= 24576, i.e. 96 KB of K / V"""
    return 24576 // (Hkv * d) // 32 * 32


def s_cases(H, Hkv, d):
    """[(S, capacity)]: the tile edges, the slice count's edges, the first key of the second and of the third burst, and the largest
    S the model's rule allows.  capacity = S + G + 37 (stale rows inside and beyond the last tile); where the rule's largest
    allocation leaves no room for that (32 rows: Hkv d >= 512), the last case is S = 32 - G in a capacity of 32; (8, 128) has none."""
    ns, G = nslice(Hkv), H // Hkv
    out = []
    for S in (1, 31, 32, 33, 32 * ns - 1, 32 * ns, 32 * ns + 1, 32 * ns * tb(d) + 1, 32 * ns * 2 * tb(d) + 1):
        if (S, S + G + 37) not in out:
            out.append((S, S + G + 37))
    sa = model_max_sa(Hkv, d)
    if sa - G - 37 >= 1:
        out.append((sa - G - 37, sa))
    elif sa - G >= 1:
        out.append((sa - G, sa))
    return out


def model_rule_case(S, capacity, Hkv, d):
    return (capacity + 31) // 32 * 32 <= model_max_sa(Hkv, d)


# ---- reference -------------------------------------------------------------------------------------------------------------------
def reference(q, k, v, w_o, S, H, Hkv, d, dtype=np.float64):
    """q [H d], k / v [rows >= S, Hkv d], w_o [N, H d]: float arrays.  (out [N], x [H d], A [H d]) in `dtype`: x the attention
    over the first S keys (test_gpu_attention_ops.reference), out = w_o . x, A = sum_j p_j |v_j|."""
    q, k, v = np.asarray(q).reshape(1, -1), np.asarray(k)[:S], np.asarray(v)[:S]
    x = attn_reference(q, k, v, S - 1, H, Hkv, d, -1, dtype=dtype)[0]
    A = attn_reference(q, k, np.abs(v), S - 1, H, Hkv, d, -1, dtype=dtype)[0]
    return np.asarray(w_o).astype(dtype) @ x, x, A


def bound(q, k, v, w_o, S, H, Hkv, d):
    """(reference out [N] fp64, bound B [N], x [K], E [K]) -- the derivation is in the module docstring"""
    q, k, v = np.asarray(q).reshape(1, -1), np.asarray(k)[:S], np.asarray(v)[:S]
    ref, x, A = reference(q, k, v, w_o, S, H, Hkv, d)
    _, f = ac.f32_bound(q, k, v, S - 1, H, Hkv, d)
    tps = -(-(-(-S // 32)) // nslice(Hkv))
    E = 2.0 ** -9 * A + 2.0 ** -9 * (np.abs(x) + 2.0 ** -9 * A) + f + (tps + 3) * 2.0 ** -24 * A
    W = np.abs(np.asarray(w_o).astype(np.float64))
    K = H * d
    return ref, W @ E + (K / 2 + 8) * 2.0 ** -24 * (W @ (np.abs(x) + E)), x, E


def dot_bound(w_o, x, K):
    """the dot-product term alone, for an x both sides share"""
    return (K / 2 + 8) * 2.0 ** -24 * (np.abs(np.asarray(w_o).astype(np.float64)) @ np.abs(x))


# ---- emulation ---------------------------------------------------------------------------------------------------------------------
def emulate_x(q, k, v, S, H, Hkv, d, pad=0.0, mistake=None, dropped_slice=1):
    """the kernel's x [H d] (float32, bf16-representable): float32 arithmetic with the kernel's rounding points and tile order.
    k / v [rows >= S, Hkv d]; the rows behind them, to the end of the last tile, hold `pad`."""
    assert mistake in (None,) + MISTAKES
    f32 = np.float32
    ns, G = nslice(Hkv), H // Hkv
    rows = max(k.shape[0], (S + 31) // 32 * 32)
    kk, vv = np.full((rows, Hkv, d), pad, f32), np.full((rows, Hkv, d), pad, f32)
    kk[:k.shape[0]] = np.asarray(k, f32).reshape(-1, Hkv, d)
    vv[:v.shape[0]] = np.asarray(v, f32).reshape(-1, Hkv, d)
    qq = np.asarray(q, f32).reshape(H, d)
    scale = f32(1.0) / np.sqrt(f32(d))
    hi = S - 1 if mistake == "drop_last_key" else S
    x = np.zeros((H, d), f32)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for hk in range(Hkv):
            src = (hk + 1) % Hkv if mistake == "kv_head" else hk
            qg = qq[hk * G:(hk + 1) * G]
            m, l, O = np.full((ns, G), -np.inf, f32), np.zeros((ns, G), f32), np.zeros((ns, G, d), f32)
            for sl in range(ns):
                for t in range(sl, (S + 31) // 32, ns):
                    key = np.arange(32 * t, 32 * t + 32)
                    sc = (qg @ kk[key, src].T) * scale                                   # [G, 32] float32
                    if mistake != "no_mask":
                        sc = np.where(key[None, :] < hi, sc, f32(-np.inf))
                    mn = np.maximum(m[sl], sc.max(axis=1))
                    dead = mn == -np.inf
                    alpha = np.where(dead, f32(1), np.exp(m[sl] - mn)).astype(f32)
                    p = np.where(dead[:, None], f32(0), np.exp(sc - mn[:, None])).astype(f32)
                    l[sl] = l[sl] * alpha + p.sum(axis=1, dtype=f32)
                    m[sl] = mn
                    O[sl] = O[sl] * alpha[:, None] + ac.bf16r(p) @ vv[key, src]
            M = m.max(axis=0)
            L, Om = np.zeros(G, f32), np.zeros((G, d), f32)
            for z in range(ns):
                if mistake == "drop_slice" and z == dropped_slice:
                    continue
                wt = np.where(m[z] == -np.inf, f32(0), np.exp(m[z] - M)).astype(f32)
                L = l[z] * wt + L
                Om = O[z] * wt[:, None] + Om
            x[hk * G:(hk + 1) * G] = ac.bf16r(Om * (f32(1) / L)[:, None])
    return x.reshape(-1)


def emulate(q, k, v, w_o, S, H, Hkv, d, pad=0.0, mistake=None, dropped_slice=1):
    """out [N] float32 of the emulated kernel.  Deliberate mistakes: drop_last_key (S - 1 keys), drop_slice (slice `dropped_slice`
    of every head is left out of the merge), kv_head (the wave reads the next kv head), row (with two rows per wave, N > 2048, row
    n is computed from W_o row n + 1, clamped), no_mask (the stale keys of the last tile take part)."""
    x = emulate_x(q, k, v, S, H, Hkv, d, pad, mistake, dropped_slice)
    w = np.asarray(w_o, np.float32)
    if mistake == "row" and rpw(w.shape[0]) == 2:
        w = w[np.minimum(np.arange(w.shape[0]) + 1, w.shape[0] - 1)]
    return w @ x


# ---- exact cases -------------------------------------------------------------------------------------------------------------------
def targets(S, Hkv, d):
    """key 0, key S - 1, both sides of every 32-key tile edge up to 2 nslice TB + 1 tiles, the first key of every slice's first tile
    and of its first tile in the second burst"""
    ns, TB = nslice(Hkv), tb(d)
    t = {0, S - 1}
    for mth in range(1, 2 * ns * TB + 2):
        t |= {32 * mth - 1, 32 * mth}
    for sl in range(ns):
        t |= {32 * sl, 32 * (sl + ns * TB)}
    return sorted(p for p in t if 0 <= p < S)


def selectors(seed, S, H, Hkv, d):
    """the decode selectors of one (layout, S): every target is some head's target in one of them (asserted by decode_selectors),
    every decoy class is present and the score gap holds (asserted here)"""
    sels = ac.decode_selectors(seed, S, H, Hkv, d, targets(S, Hkv, d))
    for sel in sels:
        assert set(sel.decoys) == ac.decode_decoy_classes(S, Hkv), sorted(sel.decoys)
        worst, ok = sel.margin()
        assert ok and worst < -ac.GAP, worst
    return sels


def owner_slice(key, Hkv):
    return (key // 32) % nslice(Hkv)


_W = {}


def _cached(key, make):
    if key not in _W:
        if len(_W) >= 20:                                   # (one layout's matrices: 8 row counts x 2 forms + the random one)
            _W.clear()
        _W[key] = make()
    return _W[key]


def sign_select_w(N, K, seed):
    """(W [N, K] float32, col [N]): row n holds +-2^e (e in -3..3) at column (n + off) % K and zeros"""
    def make():
        rs = np.random.RandomState(seed)
        col = (np.arange(N) + rs.randint(K)) % K
        w = np.zeros((N, K), np.float32)
        w[np.arange(N), col] = rs.choice([-1.0, 1.0], N) * 2.0 ** rs.randint(-3, 4, N)
        return w, col
    return _cached(("sel", N, K, seed), make)


def int_w(N, K, seed):
    return _cached(("int", N, K, seed), lambda: np.random.RandomState(seed).randint(-2, 3, (N, K)).astype(np.float32))


def int_v(sel, seed):
    """the selector's V replaced by integers in -16..16 (V takes no part in the scores)"""
    return np.random.RandomState(seed).randint(-16, 17, sel.v.shape).astype(np.float32)


def exact_forms(sel, N, seed):
    """[(name, v [rows, Hkv, d], W [N, K], want [N] float32, describe(n) -> str)] for one selector: whatever the order of the sums,
    out must equal `want` bit for bit"""
    H, d = sel.q.shape[1], sel.q.shape[2]
    K, G = H * d, H // sel.k.shape[1]
    hk = np.arange(H) // G

    def where(col):
        return "column %d = head %d (kv head %d, target key %d) element %d" % (col, col // d, col // d // G, sel.pi[0, col // d], col % d)
    w, col = sign_select_w(N, K, seed)
    x = sel.v[sel.pi[0], hk, :].reshape(-1)
    forms = [("sign-select", sel.v, w, w[np.arange(N), col] * x[col], lambda n: where(int(col[n])))]
    vi = int_v(sel, seed)
    wi = int_w(N, K, seed)
    xi = vi[sel.pi[0], hk, :].reshape(-1)
    want = (wi.astype(np.int64) @ xi.astype(np.int64)).astype(np.float32)
    forms.append(("integers", vi, wi, want, lambda n: "a sum over every head"))
    return forms


def first_difference(got, want):
    """index of the first element whose bits differ, or None"""
    bad = np.flatnonzero(np.asarray(got, np.float32).view(np.uint32) != np.asarray(want, np.float32).view(np.uint32))
    return int(bad[0]) if bad.size else None


# ---- random cases --------------------------------------------------------------------------------------------------------------------
def random_seed(d, H, Hkv, S):
    return S * 131 + d + 7 * H + Hkv


def random_w(d, H, Hkv):
    """W_o [max N, K] N(0, 1) rounded to bf16 of one layout: a case with N rows takes the first N"""
    N, K = max(n_list(d, H, Hkv)), H * d
    return _cached(("rnd", d, H, Hkv), lambda: ac.bf16r(np.random.RandomState(1000 + d + 7 * H + Hkv).standard_normal((N, K))))


def random_inputs(d, H, Hkv, S):
    """q [1, H d], k / v [S, Hkv d] float32, bf16-representable (attn_cases.random_case)"""
    return ac.random_case(random_seed(d, H, Hkv, S), 1, S, H, Hkv, d, "bf16")
