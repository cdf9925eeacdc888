"""attn_prefill_packed_mfma_kernel ALONE, through fl_op_attention_packed: ragged packs of sequences, each over a cache of its own,
against the fp64 reference of the single-sequence op tests per sequence, under the bound those tests use (test_gpu_attention_ops.check:
max error <= 1.2e-2 * scale, rel. L2 <= 5e-3).  Cache geometry that catches a wrong base or stride: seq_alloc differs per member,
the launch reads layer 1 of two (layer 0 holds other data), two stale rows follow every member's keys, everything behind holds 1e4.
Isolation: a member's output rows are bit-identical packed alone and packed among the others, wherever in the pack it sits.
The shared body (attn_prefill16.h): a member packed alone has the bits of the single-prompt 16-row kernel on the same sequence."""
import numpy as np
import pytest

import attn_cases
import synth
from test_gpu_attention_ops import check, make, reference

pytestmark = pytest.mark.gpu

SHAPES = [(2, 2), (4, 2), (6, 2), (8, 1), (32, 8)]               # (H, Hkv): G = 1, 2, 3, 8, 4
RAGGED = ([1, 15, 16, 17, 33, 48, 2], [0, 5, 32, 37, 0, 64, 31])
PACKS = {
    "ragged": RAGGED + (-1,),
    "ragged_window5": RAGGED + (5,),
    "one_of_100": ([100], [0], -1),
    "64_short": ([1 + (i * 5) % 3 for i in range(64)], [(i * 7) % 30 for i in range(64)], -1),
    # 64 members of 65 .. 94 tokens: enough items for several token sub-tiles per workgroup (TT 2 .. 4 at 1 .. 4 query heads per kv
    # head, see expected_tt), while a member packed alone gets TT = 1.  Every other member has no cached prefix, so with the window
    # its later waves start at a key tile (wstart) behind the workgroup's first staged tile (kstart), an ODD number of tiles behind
    # for the wave at token 48: the wave pair's alternation is then counted from another tile than the workgroup's.
    "64_wide_window5": ([65 + (i * 7) % 30 for i in range(64)], [0 if i % 2 == 0 else (i * 5) % 40 for i in range(64)], 5),
}


def expected_tt(H, Hkv, d, counts):
    """plan_attn_prefill_packed (attn_prefill_plan.h) restated: token sub-tiles per workgroup at the default switches"""
    G = H // Hkv
    fits2 = lambda tt: G * tt * 2 <= 16 and G * tt * (16 * d + 32) * 4 <= 64 * 1024
    tt = 16 // G if G <= 4 else 1
    while fits2(1) and tt > 1 and not fits2(tt):
        tt >>= 1
    items = lambda t: sum(-(-c // (16 * t)) for c in counts)
    while tt > 1 and (items(tt) * Hkv < 256 or 16 * (tt >> 1) >= max(counts)):
        tt >>= 1
    return tt


PAD, STALE = 1e4, 2


@pytest.fixture(scope="module")
def fa():
    import fastllm_amd
    assert fastllm_amd.device_count() >= 1
    return fastllm_amd


def geometry(counts, past):
    """rows (keys + two stale rows) and seq_alloc of every member: the smallest multiple of 32 that holds the rows, every other
    member one tile more -- 32 .. 160"""
    rows = [p + c + STALE for c, p in zip(counts, past)]
    sa = [min(160, -(-r // 32) * 32 + 32 * (i % 2)) for i, r in enumerate(rows)]
    assert all(s >= r and s % 32 == 0 for s, r in zip(sa, rows)) and 32 <= min(sa) and max(sa) <= 160
    return rows, sa


_CASES = {}


def case(pack, H, Hkv, d):
    """the inputs of one (pack, shape): per member q [count, H*d], k / v [2 layers, rows, Hkv*d] (bf16 bits), and its fp64 reference
    on layer 1's keys -- made once, shared by the tests, never modified"""
    key = (pack, H, Hkv, d)
    if key not in _CASES:
        counts, past, window = PACKS[pack]
        rows, sa = geometry(counts, past)
        rs = np.random.RandomState(1000 + 31 * H + 7 * Hkv + d + len(counts))
        bits = lambda shape: synth.f32_to_bf16_bits(rs.standard_normal(shape).astype(np.float32))
        qs = [bits((c, H * d)) for c in counts]
        ks = [bits((2, r, Hkv * d)) for r in rows]
        vs = [bits((2, r, Hkv * d)) for r in rows]
        refs = [attn_cases.reference(q, k[1, :p + c], v[1, :p + c], p, H, Hkv, d, window) for q, k, v, c, p in zip(qs, ks, vs, counts, past)]
        _CASES[key] = (counts, past, window, sa, qs, ks, vs, refs)
    return _CASES[key]


def run(fa, c, order, H, Hkv, d):
    """the members `order` of case c in one launch; returns every member's rows"""
    counts, past, window, sa, qs, ks, vs, _ = c
    out = fa.op_attention_packed(np.concatenate([qs[i] for i in order]), [ks[i] for i in order], [vs[i] for i in order], [counts[i] for i in order],
                                 [past[i] for i in order], [sa[i] for i in order], H, Hkv, d, layer=1, window=window, pad_value=PAD)
    cuts = np.cumsum([counts[i] for i in order])[:-1]
    return dict(zip(order, np.split(out, cuts)))


@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("H,Hkv", SHAPES)
@pytest.mark.parametrize("pack", list(PACKS))
def test_packed_attention_matches_reference(fa, pack, H, Hkv, d):
    c = case(pack, H, Hkv, d)
    counts, past, window, sa, _, _, _, refs = c
    got = run(fa, c, list(range(len(counts))), H, Hkv, d)
    for i, ref in enumerate(refs):
        assert got[i].shape == ref.shape
        assert not np.isnan(got[i]).any(), "member %d: an element keeps the 0xff pattern" % i       # completeness
        check(got[i], ref, "%s d=%d H=%d Hkv=%d member %d (%d new, %d cached, seq_alloc %d, window %d)" % (pack, d, H, Hkv, i, counts[i], past[i], sa[i], window))


@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("H,Hkv", SHAPES)
@pytest.mark.parametrize("pack", ["ragged", "ragged_window5", "64_short", "64_wide_window5"])
def test_a_member_does_not_depend_on_the_pack(fa, pack, H, Hkv, d):
    c = case(pack, H, Hkv, d)
    counts, n = c[0], len(c[0])
    if pack == "64_wide_window5":
        # the pack really runs several sub-tiles per workgroup where the head shape allows it, a member alone never does
        want = {(2, 2): 4, (4, 2): 4 if d == 64 else 2, (6, 2): 2, (8, 1): 1, (32, 8): 2 if d == 64 else 1}[(H, Hkv)]
        assert expected_tt(H, Hkv, d, counts) == want and all(expected_tt(H, Hkv, d, [x]) == 1 for x in counts)
    full = run(fa, c, list(range(n)), H, Hkv, d)
    moved = run(fa, c, list(range(n))[::-1], H, Hkv, d)                 # every member at another position, behind other neighbours
    rot = run(fa, c, [(i + 3) % n for i in range(n)], H, Hkv, d)
    for i in range(n):
        assert full[i].tobytes() == moved[i].tobytes() == rot[i].tobytes(), "%s member %d changes with its place in the pack" % (pack, i)
    for i in range(n):                                                  # ... and alone
        alone = run(fa, c, [i], H, Hkv, d)
        assert alone[i].tobytes() == full[i].tobytes(), "%s member %d differs packed alone" % (pack, i)


@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("H,Hkv", [(2, 2), (6, 2), (8, 1), (32, 8)])
@pytest.mark.parametrize("T,cached,window", [(17, 0, -1), (48, 37, -1), (100, 0, 5), (70, 129, 17)])
def test_a_member_alone_has_the_bits_of_the_single_prompt_kernel(fa, T, cached, window, H, Hkv, d):
    """fl_op_attention's 16-row kernel (kernel=2) and fl_op_attention_packed on one sequence: one device body, and at these lengths one
    plan -- both run one token sub-tile per workgroup (TT = 1) with the same key split and ring depth, and at TT = 1 a wave's first
    useful tile is the workgroup's first staged tile, so the two origins of the wave pair's alternation agree for any window."""
    q, k, v = make(T, cached, H, Hkv, d, seed=4000 + 13 * T + H + d)
    single = fa.op_attention(q, k, v, cached, H, Hkv, d, window=window, kernel=2)
    alone = fa.op_attention_packed(q, [k[None]], [v[None]], [T], [cached], [-(-(cached + T) // 32) * 32], H, Hkv, d, layer=0, window=window)
    assert not np.isnan(single).any() and not np.isnan(alone).any()
    check(single, reference(q, k, v, cached, H, Hkv, d, window), "single T=%d cached=%d window=%d" % (T, cached, window))
    assert single.tobytes() == alone.tobytes(), "max difference %g" % np.abs(single - alone).max()
