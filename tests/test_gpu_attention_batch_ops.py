"""The two batched decode attention kernels ALONE -- attn_decode_batch_kernel (plain layout, fp32 / bf16) and
attn_decode_mfma_batch_kernel (the production batched decode) -- through fl_op_attention_batch: every sequence a cache of its own
with its own length, capacity and split count, two layers with the launch on the second, stale rows behind every cached length.
The model-level tests run them on caches of 96 positions, where no sequence is longer than one split.

Exact selector cases (attn_cases.py), launched at successive target assignments until every sequence has had every position
where ITS split indexing can break as some head's target (asserted); decoys, asserted present: the stale tail, the next kv head
(len > 1), ANOTHER SEQUENCE of the batch (sequences with a key to spare) and the sequence's OTHER LAYER.  Random cases against
fp64.  Three relations: a batch sequence equals the single-sequence entry bit for bit where both run the same template (the
4-wave forms: plain kernels at attn_nw = 4, MFMA kernels from two splits); the first, the last and the longest sequence's output
does not change by a bit when every other sequence's K, V and length are replaced; a stale tail of 3e4 instead of 0 changes no
bit.  Every sequence names its split count, except one that takes the cache's own rule and is held against the single-sequence
entry taking the same rule from the library."""
import numpy as np
import pytest

import attn_cases as ac
from test_gpu_attention_ops import check, reference

pytestmark = pytest.mark.gpu

STALE = 3e4
LENGTHS = [1, 31, 33, 127, 129, 640, 1025, 2600]      # 2600: seq_alloc > 2560, the MFMA cache's 256-key split rule
BATCH_LENS = {1: [640], 2: [129, 1025], 3: [1, 640, 2600], 8: LENGTHS, 17: LENGTHS + [129, 33, 640, 1, 127, 31, 129, 33, 127]}
# every sequence names its split count (second table: the second half of the 17); short sequences with many splits own empty ones
NSPLIT = {1: 2, 31: 1, 33: 3, 127: 9, 129: 2, 640: 5, 1025: 17, 2600: 41}
NSPLIT_2 = {1: 1, 31: 4, 33: 1, 127: 48, 129: 5, 640: 10}
RATIOS = {}


@pytest.fixture(scope="module")
def fa():
    import fastllm_amd
    assert fastllm_amd.device_count() >= 1
    fastllm_amd.tune("attn_nw", 4)
    yield fastllm_amd
    fastllm_amd.tune("attn_batch_wgs", 256)
    for kind, rows in sorted(RATIOS.items()):
        print("batch %s kernel: largest err / bound %.3f (%s) over %d checks" % ((kind,) + max(rows) + (len(rows),)))


def geometry(B, Hkv, mfma, wgs):
    """per sequence: len (stale rows are added by the caller), seq_alloc (different slack per sequence), the nsplit argument, and
    the split count the kernel must end up with: the MFMA launch caps it at attn_batch_wgs / (Hkv * B) -- the rule under test,
    so the test states it.  Where no cap bites, ONE long sequence passes nsplit = 0 (the cache's own rule): its count is not
    restated here (None) -- it is held against the single-sequence entry, which asks the library for the same rule."""
    lens = BATCH_LENS[B]
    sa = [(n + 16 + 7 + 45 * (b % 4) + 31) // 32 * 32 for b, n in enumerate(lens)]        # (16: room for the stale rows)
    arg = [(NSPLIT if b < 8 else NSPLIT_2)[n] for b, n in enumerate(lens)]
    cap = max(1, wgs // (Hkv * B)) if mfma else 64
    eff = [min(a, cap) for a in arg]
    if cap >= 48:
        auto = lens.index(640) if 640 in lens else lens.index(1025)
        arg[auto], eff[auto] = 0, None
    return lens, sa, arg, eff


def batch_targets(n, eff, d, mfma):
    """decode_targets by the sequence's split length; for the nsplit = 0 sequence both sides of every multiple of 16 keys (every
    split length of either kernel is one)"""
    if eff is not None:
        return ac.decode_targets(n, eff, d, 4, layout=int(mfma))
    return sorted({0, n - 1} | {p for m in range(16, n, 16) for p in (m - 1, m)})


_RANDOM = {}


def random_batch(B, H, Hkv, d, dtype):
    """q [B, H*d], per sequence K / V [2, len, Hkv*d] (float32 values; bf16-representable for 'bf16'), the fp64 reference of layer
    1 and its fp32 bound: made once per shape and shared"""
    key = (B, H, Hkv, d, dtype)
    if key not in _RANDOM:
        lens = BATCH_LENS[B]
        rs = np.random.RandomState(B * 1000 + H + d)
        rnd = (lambda *s: ac.bf16r(rs.standard_normal(s))) if dtype == "bf16" else (lambda *s: rs.standard_normal(s).astype(np.float32))
        q = rnd(B, H * d)
        ks, vs = [rnd(2, n, Hkv * d) for n in lens], [rnd(2, n, Hkv * d) for n in lens]
        refs = [ac.f32_bound(q[b:b + 1], ks[b][1], vs[b][1], lens[b] - 1, H, Hkv, d) for b in range(B)]
        _RANDOM[key] = (q, ks, vs, refs)
    return _RANDOM[key]


def batch_selector(seed, lens, targets, H, Hkv, d, shift):
    """One decode selector per sequence, then the decoys only a batch has: sequence b's first query code at twice the magnitude on
    a key of sequence b + 1 that is no target, and -- in layer 0, which the launch on layer 1 must not read -- every query head's
    code at its target's own position.  Returns (selectors, layer-0 K / V per sequence)."""
    B, G = len(lens), H // Hkv
    for attempt in range(16):
        sels = [ac.decode_selector(seed * 1009 + attempt * 101 + b, lens[b], H, Hkv, d, targets[b], shift=shift + b * G) for b in range(B)]
        for b in range(B if B > 1 else 0):
            nb = (b + 1) % B
            busy = set(sels[nb].pi[0]) | {pos for rows in sels[nb].decoys.values() for pos, hk, _, _ in rows if hk == 0}
            free = [p for p in range(lens[nb]) if p not in busy]
            if free:
                sels[nb].k[free[0], 0] = 2.0 * sels[b].q[0, 0]
                sels[nb].decoys.setdefault("sequence", []).append((free[0], 0, b, 0))
        if all(ok and worst < -ac.GAP for worst, ok in (s.margin() for s in sels)):
            break
    else:
        raise AssertionError("no seed gives the batch its score gap")
    rs = np.random.RandomState(seed + 5)
    other = []
    for s in sels:
        k0 = rs.choice([-8.0, 8.0], size=s.k.shape).astype(np.float32)
        v0 = ac.bf16r(rs.standard_normal(s.v.shape))
        for h in range(H):
            k0[s.pi[0, h], h // G] = 2.0 * s.q[0, h]
            s.decoys.setdefault("layer", []).append((int(s.pi[0, h]), h // G, 0, h))
        other.append((k0, v0))
    return sels, other


KINDS = [("f32", 0, 256), ("bf16", 0, 256), ("bf16", 1, 16), ("bf16", 1, 256), ("bf16", 1, 4096)]


@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("H,Hkv", [(12, 4), (28, 4)])
@pytest.mark.parametrize("B", [1, 2, 3, 8, 17])
@pytest.mark.parametrize("dtype,layout,wgs", KINDS)
def test_batch(fa, d, H, Hkv, B, dtype, layout, wgs):
    mfma, G = layout == 1, H // Hkv
    kind = "mfma" if mfma else "plain " + dtype
    what = "batch %s d=%d H=%d Hkv=%d B=%d wgs=%d" % (kind, d, H, Hkv, B, wgs)
    fa.tune("attn_batch_wgs", wgs)
    lens, sa, arg, eff = geometry(B, Hkv, mfma, wgs)
    common = dict(layout=layout, layer=1)

    # ---- exact: as many launches as it takes for every target of every sequence to have been some head's target
    targets = [batch_targets(lens[b], eff[b], d, mfma) for b in range(B)]
    seen = [set() for _ in range(B)]
    for it in range(max(len(t) for t in targets) + 2):
        sels, other = batch_selector(B * 31 + d + H + wgs, lens, targets, H, Hkv, d, it * H)
        for b, s in enumerate(sels):
            worst, ok = s.margin()
            assert ok and worst < -ac.GAP, (what, worst)
            want_classes = ac.decode_decoy_classes(lens[b], Hkv) | {"layer"} | ({"sequence"} if B > 1 and lens[b] > H + 2 else set())
            assert want_classes <= set(s.decoys), (what, b, sorted(s.decoys))
            seen[b] |= set(int(p) for p in s.pi.ravel())
        q = np.concatenate([s.q.reshape(1, -1) for s in sels])
        ks = [np.stack([o[0], s.k]).reshape(2, s.k.shape[0], -1) for s, o in zip(sels, other)]
        vs = [np.stack([o[1], s.v]).reshape(2, s.v.shape[0], -1) for s, o in zip(sels, other)]
        got = fa.op_attention_batch(ac.as_input(q, dtype), [ac.as_input(a, dtype) for a in ks], [ac.as_input(a, dtype) for a in vs], lens, sa,
                                    arg, H, Hkv, d, pad_value=STALE, repeat=3, **common)
        want = np.concatenate([s.expected() for s in sels])
        for r in range(3):
            bad = np.argwhere(got[r] != want)
            assert bad.size == 0, "%s selector, launch %d: %d elements differ, first at sequence %d (len %d, %s splits) head %d (target key %d)" % (
                what, r, len(bad), bad[0][0], lens[bad[0][0]], eff[bad[0][0]], bad[0][1] // d, sels[bad[0][0]].pi[0, bad[0][1] // d])
        if all(seen[b] >= set(targets[b]) for b in range(B)):
            break
    assert all(seen[b] == set(targets[b]) for b in range(B)), what + ": targets never taken"

    # ---- random data against fp64
    qf, kf, vf, refs = random_batch(B, H, Hkv, d, dtype)
    qi, ki, vi = ac.as_input(qf, dtype), [ac.as_input(a, dtype) for a in kf], [ac.as_input(a, dtype) for a in vf]
    got = fa.op_attention_batch(qi, ki, vi, lens, sa, arg, H, Hkv, d, repeat=3, **common)
    for b in range(B):
        tag = "%s sequence %d (len %d, %s splits)" % (what, b, lens[b], eff[b])
        if mfma:
            # the bar of test_gpu_attention_ops.check, unchanged; its two ratios are printed and kept for the module's summary
            e, ref = np.abs(got[0, b:b + 1] - refs[b][0]), refs[b][0]
            ratio = max(e.max() / (1.2e-2 * max(1e-6, np.abs(ref).max())),
                        np.linalg.norm(got[0, b:b + 1] - ref) / max(1e-30, np.linalg.norm(ref)) / 5e-3)
            RATIOS.setdefault("mfma", []).append((float(ratio), tag))
            print("%s: worst of (max err, rel L2) / bar %.3f" % (tag, ratio))
            check(got[0, b:b + 1], ref, tag)
        else:
            ac.check_plain(got[0, b:b + 1], refs[b][0], refs[b][1], dtype, tag, RATIOS)
    for r in (1, 2):
        assert (got[r].view(np.uint32) == got[0].view(np.uint32)).all(), "%s: launch %d differs from launch 0" % (what, r)

    # ---- same template, same bits: the single-sequence entry at the split count the batch kernel must end up with (the nsplit = 0
    # sequence: at nsplit = 0, the library's own rule for a cache of that capacity)
    for b in range(B):
        if mfma and eff[b] is not None and eff[b] < 2:
            continue                                     # (one split: the single-sequence launch is the 16-wave form)
        one = fa.op_attention_plain(qi[b:b + 1], ki[b][1], vi[b][1], lens[b] - 1, H, Hkv, d, layout=layout, kernel=1, nsplit=eff[b] or 0,
                                    capacity=sa[b])[0]
        assert (one.view(np.uint32) == got[0, b:b + 1].view(np.uint32)).all(), \
            "%s sequence %d (len %d, %s splits): differs from the single-sequence kernel" % (what, b, lens[b], eff[b])

    # ---- stale tail
    pad = fa.op_attention_batch(qi, ki, vi, lens, sa, arg, H, Hkv, d, pad_value=STALE, **common)
    assert (pad[0].view(np.uint32) == got[0].view(np.uint32)).all(), what + ": the stale tail changed the output"

    # ---- neighbour independence: every other sequence gets new K, V and a new length; kept in turn: the first sequence, the last
    # and the longest
    for keep in sorted({0, B - 1, int(np.argmax(lens))}) if B > 1 else ():
        rs = np.random.RandomState(B + d + keep)
        lens2 = [n if b == keep else max(1, n // 2 + 1) for b, n in enumerate(lens)]
        k2 = [ki[b] if b == keep else ac.as_input(ac.bf16r(rs.standard_normal((2, lens2[b], Hkv * d))), dtype) for b in range(B)]
        v2 = [vi[b] if b == keep else ac.as_input(ac.bf16r(rs.standard_normal((2, lens2[b], Hkv * d))), dtype) for b in range(B)]
        nb = fa.op_attention_batch(qi, k2, v2, lens2, sa, arg, H, Hkv, d, **common)
        assert (nb[0, keep].view(np.uint32) == got[0, keep].view(np.uint32)).all(), "%s: sequence %d changed with its neighbours" % (what, keep)


@pytest.mark.parametrize("H,Hkv", [(18, 2), (24, 2), (16, 1)])
def test_mfma_batch_refuses_more_than_8_heads_per_kv_head(fa, H, Hkv):
    q, k, v = (ac.as_input(a, "bf16") for a in ac.random_case(2, 1, 5, H, Hkv, 64, "bf16"))
    with pytest.raises(fa.FastLLMError) as e:
        fa.op_attention_batch(q, [k[None]], [v[None]], [5], [32], [0], H, Hkv, 64, layout=1)
    assert e.value.code == -10                                               # FL_ERR_UNSUPPORTED
    got = fa.op_attention_batch(q, [k[None]], [v[None]], [5], [32], [0], H, Hkv, 64, layout=0)   # ... the plain kernel takes them
    check(got[0], reference(q, k, v, 4, H, Hkv, 64, -1), "plain batch G=%d" % (H // Hkv))
