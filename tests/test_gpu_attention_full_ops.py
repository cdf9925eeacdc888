"""The FULL-mask instantiations of attn_prefill_packed_mfma_kernel ALONE, through fl_op_attention_packed_ex with mask = 1: every new
token of a member sees all of the member's keys.  Reference: a float64 softmax over all of a member's keys, under
test_gpu_attention_ops.check, the bound of the causal op tests.  Packs without a cached prefix (the full mask needs an empty cache):
the ragged one -- 1, 15, 16, 17 tokens around the 16-row tile, 33 and 48 with two and three tiles, 100 with a last key tile of four
keys -- and 64 members of 65 .. 94 tokens, where several token sub-tiles share a workgroup.  The cache geometry of
test_gpu_packed_attention.py: seq_alloc differs per member, the launch reads layer 1 of two, two stale rows follow every member's
keys and everything behind holds 1e4 -- a key range that runs past len + T reads them.  A member's bits do not depend on the pack;
mask = 0 through the _ex entry has the bits of fl_op_attention_packed."""
import numpy as np
import pytest

import synth
import test_gpu_packed_attention as causal
from test_gpu_attention_ops import check

pytestmark = pytest.mark.gpu

SHAPES = [(2, 2), (6, 2), (8, 1), (32, 8)]
PACKS = {
    "ragged": [1, 15, 16, 17, 33, 48, 2, 100],
    "64_wide": [65 + (i * 7) % 30 for i in range(64)],
}
PAD = causal.PAD


@pytest.fixture(scope="module")
def fa():
    import fastllm_amd
    assert fastllm_amd.device_count() >= 1
    return fastllm_amd


def full_reference(q, k, v, H, Hkv, d):
    """float64 softmax of every query over ALL keys; q [T, H*d], k / v [T, Hkv*d] bf16 bits"""
    wide = lambda a: synth.bf16_bits_to_f32(a).astype(np.float64)
    qf, kf, vf = wide(q).reshape(-1, H, d), wide(k).reshape(-1, Hkv, d), wide(v).reshape(-1, Hkv, d)
    G = H // Hkv
    out = np.zeros(qf.shape)
    for h in range(H):
        sc = qf[:, h, :] @ kf[:, h // G, :].T / np.sqrt(d)
        p = np.exp(sc - sc.max(axis=1, keepdims=True))
        out[:, h, :] = (p / p.sum(axis=1, keepdims=True)) @ vf[:, h // G, :]
    return out.reshape(qf.shape[0], H * d)


_CASES = {}


def case(pack, H, Hkv, d):
    """per member q [count, H*d], k / v [2 layers, count + 2 stale rows, Hkv*d] (bf16 bits) and the float64 reference on layer 1's
    keys -- made once, shared by the tests, never modified"""
    key = (pack, H, Hkv, d)
    if key not in _CASES:
        counts = PACKS[pack]
        past = [0] * len(counts)
        rows, sa = causal.geometry(counts, past)
        rs = np.random.RandomState(2000 + 31 * H + 7 * Hkv + d + len(counts))
        bits = lambda shape: synth.f32_to_bf16_bits(rs.standard_normal(shape).astype(np.float32))
        qs = [bits((c, H * d)) for c in counts]
        ks = [bits((2, r, Hkv * d)) for r in rows]
        vs = [bits((2, r, Hkv * d)) for r in rows]
        refs = [full_reference(q, k[1, :c], v[1, :c], H, Hkv, d) for q, k, v, c in zip(qs, ks, vs, counts)]
        _CASES[key] = (counts, past, sa, qs, ks, vs, refs)
    return _CASES[key]


def run(fa, c, order, H, Hkv, d, window=-1):
    counts, past, sa, qs, ks, vs, _ = c
    out = fa.op_attention_packed(np.concatenate([qs[i] for i in order]), [ks[i] for i in order], [vs[i] for i in order], [counts[i] for i in order],
                                 [past[i] for i in order], [sa[i] for i in order], H, Hkv, d, layer=1, window=window, pad_value=PAD, mask=1)
    cuts = np.cumsum([counts[i] for i in order])[:-1]
    return dict(zip(order, np.split(out, cuts)))


@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("H,Hkv", SHAPES)
@pytest.mark.parametrize("pack", list(PACKS))
def test_full_mask_matches_reference(fa, pack, H, Hkv, d):
    c = case(pack, H, Hkv, d)
    counts, sa, refs = c[0], c[2], c[6]
    got = run(fa, c, list(range(len(counts))), H, Hkv, d)
    for i, ref in enumerate(refs):
        assert got[i].shape == ref.shape
        assert not np.isnan(got[i]).any(), "member %d: an element keeps the 0xff pattern" % i
        check(got[i], ref, "%s d=%d H=%d Hkv=%d member %d (%d tokens, seq_alloc %d)" % (pack, d, H, Hkv, i, counts[i], sa[i]))
    if pack == "ragged":
        # the window is ignored under the full mask
        win = run(fa, c, list(range(len(counts))), H, Hkv, d, window=5)
        assert all(win[i].tobytes() == got[i].tobytes() for i in range(len(counts)))
        # ... and the mask is really off: row 0 of the 17-token member is not its causal value (its own value row)
        v17 = synth.bf16_bits_to_f32(c[5][3][1, 0]).reshape(Hkv, d)
        causal_row0 = np.repeat(v17, H // Hkv, axis=0).reshape(-1)
        assert np.abs(got[3][0] - causal_row0).max() > 0.1


@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("H,Hkv", SHAPES)
@pytest.mark.parametrize("pack", list(PACKS))
def test_a_member_does_not_depend_on_the_pack(fa, pack, H, Hkv, d):
    c = case(pack, H, Hkv, d)
    counts, n = c[0], len(c[0])
    if pack == "64_wide" and (H, Hkv) != (8, 1) and not ((H, Hkv) == (32, 8) and d == 128):
        # the pack really runs several token sub-tiles per workgroup, a member alone never does
        assert causal.expected_tt(H, Hkv, d, counts) > 1 and all(causal.expected_tt(H, Hkv, d, [x]) == 1 for x in counts)
    full = run(fa, c, list(range(n)), H, Hkv, d)
    moved = run(fa, c, list(range(n))[::-1], H, Hkv, d)
    rot = run(fa, c, [(i + 3) % n for i in range(n)], H, Hkv, d)
    for i in range(n):
        assert full[i].tobytes() == moved[i].tobytes() == rot[i].tobytes(), "%s member %d changes with its place in the pack" % (pack, i)
    for i in range(0, n, 1 if n <= 8 else 9):                 # ... and alone (the 64-member pack: every ninth member)
        alone = run(fa, c, [i], H, Hkv, d)
        assert alone[i].tobytes() == full[i].tobytes(), "%s member %d differs packed alone" % (pack, i)


@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("H,Hkv", SHAPES)
def test_mask_0_through_ex_has_the_bits_of_the_plain_entry(fa, H, Hkv, d):
    counts, past, window, sa, qs, ks, vs, refs = causal.case("ragged_window5", H, Hkv, d)
    args = (np.concatenate(qs), ks, vs, counts, past, sa, H, Hkv, d)
    plain = fa.op_attention_packed(*args, layer=1, window=window, pad_value=PAD, ex=False)
    ex = fa.op_attention_packed(*args, layer=1, window=window, pad_value=PAD, mask=0, ex=True)
    assert not np.isnan(plain).any() and plain.tobytes() == ex.tobytes()
    check(ex[:counts[0]], refs[0], "member 0")
