"""Inputs and bounds shared by test_gpu_attention_plain_ops.py and test_gpu_attention_batch_ops.py.

Selector cases: keys and queries are +-8 sign codes of length d, query (t, h) carries the code of ONE visible key pi(t, h) of its
kv head, V is arbitrary bf16-representable data.  The target's score q.k / sqrt(d) = 64 sqrt(d) (512 / 724) is then more than 110
above every other visible score (checked on the inputs by `margin`), so every other softmax weight is exactly 0 in fp32 (exp(-110)
= 1.7e-48, below the smallest fp32 denormal) and in a bf16 P, the target's weight is exp(0) = 1, l = 1, and the output must equal
v[pi(t, h), kv head of h] BIT FOR BIT -- in any summation order, split count or merge order.  Decoys -- keys with a query's code at
TWICE the magnitude, at positions that query must not see -- would win the softmax outright if a kernel read them.

Random cases: the fp32 bound of the issue, 10 * e32 + (1.4427 * gmax + 2) * 2^-23 * max|v|: e32 the error of a numpy float32 run of
the same case against fp64, gmax the largest (max - score) over visible keys (__expf multiplies by log2 e in fp32 before a hardware
exp2: an absolute error of ~gmax * 1.4427 * 2^-24 in the exponent, i.e. that relative error in the weight)."""
import numpy as np

import synth
from test_gpu_attention_ops import reference

LAYOUTS = [(8, 8), (12, 4), (28, 4), (8, 1), (18, 2), (24, 2), (16, 1)]      # (H, Hkv): G = 1, 3, 7, 8, 9, 12, 16
GAP = 110.0


def bf16r(a):
    """float array rounded to bf16-representable float32 values"""
    return synth.bf16_bits_to_f32(synth.f32_to_bf16_bits(np.asarray(a, dtype=np.float32)))


def as_input(a, dtype):
    """a float32 array of bf16-representable values as the entry points take it: uint16 bits ('bf16') or float32 ('f32')"""
    a = np.ascontiguousarray(a, dtype=np.float32)
    return synth.f32_to_bf16_bits(a) if dtype == "bf16" else a


def decode_splits(S, nsplit, d, nw, layout=0):
    """(per, width): the split length as the decode kernels compute it and the keys one round of a workgroup's waves covers
    (plain: NW * KPI with KPI = 64 / (d / 8) keys per wave instruction; MFMA: 32 * NW)."""
    width = nw * (32 if layout == 1 else 64 // (d // 8))
    per = -(-S // nsplit)
    return -(-per // width) * width, width


def decode_targets(S, nsplit, d, nw, layout=0):
    """Key positions where the decode kernels' indexing can break: the ends, both sides of every split boundary, and inside the
    first and the last non-empty split both sides of every wave's key batch (KPI keys, or a 32-key MFMA tile) through the second
    round of the UNR = 2 unrolled loop."""
    per, width = decode_splits(S, nsplit, d, nw, layout)
    kpi = width // nw
    t = {0, S - 1}
    for s in range(1, nsplit):
        t |= {s * per - 1, s * per}
    for lo in (0, (S - 1) // per * per):
        for m in range(1, 2 * nw + 2):
            t |= {lo + m * kpi - 1, lo + m * kpi}
    return sorted(p for p in t if 0 <= p < S)


class Selector:
    """One sequence: q [nq, H, d], k / v [rows, Hkv, d] (float32, bf16-representable), pi [nq, H] the target key of every query,
    vis [nq, rows] the keys a query may see, decoys {class: [(pos, kv head, t, h)]}."""

    def expected(self):
        G = self.q.shape[1] // self.k.shape[1]
        hk = np.arange(self.q.shape[1]) // G
        return self.v[self.pi, hk[None, :], :].reshape(self.q.shape[0], -1)

    def margin(self):
        """the largest (score - target score) over the other visible keys, over all queries, in fp64 (must be < -GAP); and whether
        every query's best visible key is its target"""
        nq, H, d = self.q.shape
        G = H // self.k.shape[1]
        worst, ok = -np.inf, True
        for h in range(H):
            sc = self.q[:, h, :].astype(np.float64) @ self.k[:, h // G, :].astype(np.float64).T / np.sqrt(d)
            sc = np.where(self.vis, sc, -np.inf)
            ok = ok and (sc.argmax(axis=1) == self.pi[:, h]).all()
            tgt = sc[np.arange(nq), self.pi[:, h]].copy()
            sc[np.arange(nq), self.pi[:, h]] = -np.inf
            worst = max(worst, (sc.max(axis=1) - tgt).max())
        return worst, ok


_BASE = {}


def _base(seed, rows, Hkv, d):
    """the random codes and values of one seed, made once (the launches of a case differ only in their targets)"""
    key = (seed, rows, Hkv, d)
    if key not in _BASE:
        if len(_BASE) >= 24:
            _BASE.clear()
        rs = np.random.RandomState(seed)
        _BASE[key] = (rs.choice([-8.0, 8.0], size=(rows, Hkv, d)).astype(np.float32), bf16r(rs.standard_normal((rows, Hkv, d))))
    k, v = _BASE[key]
    return k.copy(), v


def selector(seed, vis, H, Hkv, d, targets, decoy_plan=(), n_stale=0, shift=0, pinned=None):
    """vis [nq, n_keys] bool.  targets: candidate key positions; query (t, h) takes the (t * H + h + shift)-th of those it may see,
    unless pinned[(t, h)] = (pos, reserve) names its target (reserve: no other query of the kv head may take pos).  n_stale rows of
    stale contents follow the n_keys keys.  decoy_plan: (class, pos, kv head, t, h) -- the key at (pos, kv head) becomes twice the
    code of query (t, h); such positions are never targets, and no query that may see one shares its owner's target (asserted).
    Seeds are tried in turn until the score gap holds (at d = 64 a decoy that OTHER queries may see has a ~1e-3 chance per query
    of coming within the gap)."""
    nq, n_keys = vis.shape
    rows, G = n_keys + n_stale, H // Hkv
    pinned = pinned or {}
    taken = {(pos, hk) for _, pos, hk, _, _ in decoy_plan}
    reserved = {(pos, h // G) for (t, h), (pos, res) in pinned.items() if res}
    assert not taken & {(pos, h // G) for (t, h), (pos, res) in pinned.items()}
    for attempt in range(64):
        s = Selector()
        s.k, s.v = _base(seed * 64 + attempt, rows, Hkv, d)
        s.vis = np.zeros((nq, rows), dtype=bool)
        s.vis[:, :n_keys] = vis
        s.pi = np.zeros((nq, H), dtype=np.int64)
        s.q = np.zeros((nq, H, d), dtype=np.float32)
        for t in range(nq):
            for hk in range(Hkv):
                cand = [p for p in targets if vis[t, p] and (p, hk) not in taken and (p, hk) not in reserved]
                for h in range(hk * G, (hk + 1) * G):
                    if (t, h) in pinned:
                        s.pi[t, h] = pinned[(t, h)][0]
                        assert vis[t, s.pi[t, h]]
                    else:
                        assert cand, "query row %d has no target in kv head %d" % (t, hk)
                        s.pi[t, h] = cand[(t * H + h + shift) % len(cand)]
                    s.q[t, h] = s.k[s.pi[t, h], hk]
        s.decoys = {}
        for cls, pos, hk, t, h in decoy_plan:
            assert not s.vis[t, pos] or hk != h // G, "decoy of class %s is visible to its own query" % cls
            assert hk != h // G or not (s.vis[:, pos, None] & (s.pi[:, hk * G:(hk + 1) * G] == s.pi[t, h])).any(), \
                "a query that may see the %s decoy shares its owner's target" % cls
            s.k[pos, hk] = 2.0 * s.q[t, h]
            s.decoys.setdefault(cls, []).append((pos, hk, t, h))
        worst, ok = s.margin()
        if ok and worst < -GAP:
            return s
    raise AssertionError("no seed gives the selector its score gap")


def decode_selector(seed, S, H, Hkv, d, targets, shift=0):
    """One decode query row (all S keys visible).  Decoys: in the stale tail one per query head (row S + g of its kv head: what a
    truncate or a rollback leaves behind the cached length), and in the NEXT kv head one per kv head (the code of the group's first
    query head) at the first key that is no target -- or, where every key is one, at a target that this kv head then gives up (a
    different one per kv head, so that the other heads still take it).  S = 1 leaves no room for the second class."""
    G = H // Hkv
    plan = [("stale", S + h % G, h // G, 0, h) for h in range(H)]
    free = [p for p in range(S) if p not in set(targets)]
    if Hkv > 1 and S > 1:
        plan += [("kv_head", free[0] if free else targets[(hk + 1) % Hkv % len(targets)], (hk + 1) % Hkv, 0, hk * G) for hk in range(Hkv)]
    return selector(seed, np.ones((1, S), dtype=bool), H, Hkv, d, targets, plan, G, shift)


def decode_selectors(seed, S, H, Hkv, d, targets):
    """decode selectors at successive shifts until EVERY target position has been some head's target (asserted): one launch takes
    H of them"""
    sels, seen = [], set()
    for it in range(len(targets) + 2):
        sels.append(decode_selector(seed, S, H, Hkv, d, targets, shift=it * H))
        seen |= set(int(p) for p in sels[-1].pi.ravel())
        if seen >= set(targets):
            break
    assert seen == set(targets), "targets never taken: %s" % sorted(set(targets) - seen)
    return sels


def decode_decoy_classes(S, Hkv):
    return {"stale"} | ({"kv_head"} if Hkv > 1 and S > 1 else set())


def prefill_visible(T, s_past, window, call0):
    p = s_past + np.arange(T)[:, None]
    j = np.arange(s_past + T)[None, :]
    return (j < call0) | ((j <= p) & ((window < 0) | (j + window >= p)))


def prefill_named_targets(T, s_past, window, call0):
    """key 0, the last key, the first in-call key, key call0 and the key before it: those that some query may see"""
    vis = prefill_visible(T, s_past, window, call0)
    return sorted(p for p in {0, s_past + T - 1, s_past, call0, max(call0 - 1, 0)} if vis[:, p].any())


def prefill_decoy_classes(T, s_past, window, call0, Hkv):
    S = s_past + T
    return ({"stale"} | ({"future"} if T >= 3 else set()) | ({"kv_head"} if Hkv > 1 and S >= 5 and T >= 2 else set())
            | ({"window"} if window >= 0 and S - 2 - window >= call0 else set()))


def prefill_selector(seed, T, s_past, window, call0, H, Hkv, d):
    """Targets: the named keys (each pinned to one query that may see it), every query's own key and the oldest key its window
    leaves.  Decoys, per kv head hk (owner: the group's first query head):
      stale    rows S + g carry the codes of the LAST query's heads (2 G rows of stale contents);
      future   key S - 2 carries the code of query T - 3, whose target is its own key S - 3, reserved for it (queries T - 2 and
               T - 1 see the decoy);
      window   the key just before the oldest one query T - 1 may see (when that is an in-call key) carries the code of query
               T - 1, whose target is its own key S - 1, which no earlier query sees;
      kv_head  key S - 4 of the NEXT kv head carries the code of query T - 1."""
    S, G = s_past + T, H // Hkv
    vis = prefill_visible(T, s_past, window, call0)
    classes = prefill_decoy_classes(T, s_past, window, call0, Hkv)
    targets = set(prefill_named_targets(T, s_past, window, call0))
    for t in range(T):
        targets |= {s_past + t, int(np.argmax(vis[t] & (np.arange(S) >= call0)))}
    plan = [("stale", S + h % G, h // G, T - 1, h) for h in range(H)]
    pinned = {}
    out = S - 2 - window
    for hk in range(Hkv):
        if "future" in classes:
            plan.append(("future", S - 2, hk, T - 3, hk * G))
            pinned[(T - 3, hk * G)] = (S - 3, True)
        if "window" in classes:
            plan.append(("window", out, hk, T - 1, hk * G))
            pinned[(T - 1, hk * G)] = (S - 1, True)
        if "kv_head" in classes:
            plan.append(("kv_head", S - 4, (hk + 1) % Hkv, T - 1, hk * G))
    taken = {(pos, hk) for _, pos, hk, _, _ in plan}
    h = H - 1
    for pos in prefill_named_targets(T, s_past, window, call0):
        t = int(np.argmax(vis[:, pos]))
        reserved = lambda h: any(p == pos and res and hh // G == h // G for (_, hh), (p, res) in pinned.items())
        while h >= 0 and ((t, h) in pinned or (pos, h // G) in taken or reserved(h)):
            h -= 1
        if h >= 0:
            pinned[(t, h)] = (pos, False)
            h -= 1
    s = selector(seed, vis, H, Hkv, d, sorted(targets), plan, 2 * G, pinned=pinned)
    assert set(s.decoys) == classes, (sorted(s.decoys), sorted(classes))
    return s


# ---- random data -------------------------------------------------------------------------------------------------------------
def random_case(seed, T, rows, H, Hkv, d, dtype):
    """q [T, H*d], k / v [rows, Hkv*d] N(0, 1): float32, or bf16-representable float32 for dtype 'bf16'"""
    rs = np.random.RandomState(seed)
    q, k, v = (rs.standard_normal(s).astype(np.float32) for s in ((T, H * d), (rows, Hkv * d), (rows, Hkv * d)))
    return (bf16r(q), bf16r(k), bf16r(v)) if dtype == "bf16" else (q, k, v)


def f32_bound(q, k, v, s_past, H, Hkv, d, window=-1, call0=None):
    """(fp64 reference, the issue's fp32 bound) of one case; k / v hold exactly the s_past + T keys"""
    ref = reference(q, k, v, s_past, H, Hkv, d, window, call0)
    e32 = np.abs(reference(q, k, v, s_past, H, Hkv, d, window, call0, dtype=np.float32).astype(np.float64) - ref).max()
    T, S, G = q.shape[0], k.shape[0], H // Hkv
    vis = prefill_visible(T, s_past, window, s_past if call0 is None else call0) if T > 1 else np.ones((1, S), dtype=bool)
    qf, kf = q.astype(np.float64).reshape(T, H, d), k.astype(np.float64).reshape(S, Hkv, d)
    gmax = 0.0
    for h in range(H):
        sc = np.where(vis, qf[:, h, :] @ kf[:, h // G, :].T / np.sqrt(d), np.nan)
        gmax = max(gmax, float(np.nanmax(np.nanmax(sc, axis=1) - np.nanmin(sc, axis=1))))
    return ref, 10 * e32 + (1.4427 * gmax + 2) * 2.0 ** -23 * float(np.abs(v).max())


def check_plain(got, ref, bound, dtype, what, ratios):
    """fp32: |got - ref| <= bound.  bf16 plain kernels (fp32 arithmetic, only the output rounded): elementwise
    |got - ref| <= 2^-8 |ref| + bound.  Prints achieved / bound and records the ratio under ratios[dtype]."""
    assert np.isfinite(got).all(), what + ": non-finite output (an element the kernel did not write?)"
    err = np.abs(got.astype(np.float64) - ref)
    lim = bound + (2.0 ** -8 * np.abs(ref) if dtype == "bf16" else 0.0)
    ratio = float((err / lim).max())
    ratios.setdefault(dtype, []).append((ratio, what))
    print("%s %s: max err %.3g, bound %.3g, worst err / bound %.3f" % (what, dtype, err.max(), bound, ratio))
    assert ratio <= 1.0, "%s %s: err / bound %.3f (max err %.3g, fp32 bound %.3g)" % (what, dtype, ratio, err.max(), bound)
