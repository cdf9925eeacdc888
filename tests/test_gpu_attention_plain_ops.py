"""The plain-layout (VALU) attention kernels of k_attn.hip ALONE -- attn_decode_kernel and attn_prefill_kernel, the attention of
every fp32 model and of every bf16 head shape the MFMA kernels refuse -- through fl_op_attention_plain, which builds the cache in
the model's layout and calls the launches the model calls.  Until now the suite saw them only through whole-model logits (1e-3
absolute in fp32, at most 3 query heads per kv head, caches of 64 positions).

Two kinds of case (attn_cases.py): exact SELECTOR cases, whose output must equal one row of V bit for bit whatever the split count
or merge order, and RANDOM cases against the fp64 reference under the derived fp32 bound.  Decode selectors are launched at
successive target assignments until EVERY position where the indexing can break has been some head's target (asserted: key 0, the
last key, both sides of every split, wave-batch and unroll boundary); decoys sit in the stale rows behind the cached length and in
the next kv head (S > 1).  Prefill selectors pin key 0, the last key, the first in-call key, key call0 and the key before it to one
query each (where any query may see them; asserted) and deal every query's own key and the oldest key of its window to the rest;
their decoys -- stale rows, a future key (T >= 3), the key just outside the last query's window (where that is an in-call key), the
next kv head (S >= 5) -- are asserted present per case.  The bf16 bound adds the output rounding, elementwise.
Shapes: more than 8 query heads per kv head (gridDim.z > 1, ragged last head group, the ticket index), the GMAX = 8 forms, the
16-wave forms behind attn_nw, the parallel combine of decode_tail (parts 2 / 4 / 8), its streaming loop, splits that own no key, a
chunked prefill's call0 < len. Every decode launch is repeated on one scratch: a ticket word that did not return to zero shows up
as a different (or unwritten) later output. The same stale-tail and call0 cases run on the MFMA single-sequence kernels (layout
1)."""
import numpy as np
import pytest

import attn_cases as ac
from test_gpu_attention_ops import check, reference

pytestmark = pytest.mark.gpu

STALE = 3e4                    # finite: the MFMA kernels multiply a masked P = 0 into V^T, and real stale rows are finite
RATIOS = {}


@pytest.fixture(scope="module")
def fa():
    import fastllm_amd
    assert fastllm_amd.device_count() >= 1
    yield fastllm_amd
    fastllm_amd.tune("attn_nw", 4)
    for dtype, rows in sorted(RATIOS.items()):
        print("plain %s kernels: largest err / bound %.3f (%s) over %d checks" % ((dtype,) + max(rows) + (len(rows),)))


def plain_nw(nw, G):
    """waves of the decode workgroup launch_attn_decode picks: 4, or behind attn_nw >= 16 sixteen (G <= 4) / eight"""
    return 4 if nw < 16 else (16 if G <= 4 else 8)


def run_decode_case(fa, d, H, Hkv, S, nsplit):
    G, what = H // Hkv, "decode d=%d H=%d Hkv=%d S=%d nsplit=%d" % (d, H, Hkv, S, nsplit)
    seed = S * 131 + nsplit * 7 + d + H
    for dtype in ("f32", "bf16"):
        q, k, v = ac.random_case(seed, 1, S, H, Hkv, d, dtype)
        ref, bound = ac.f32_bound(q, k, v, S - 1, H, Hkv, d)
        qi, ki, vi = (ac.as_input(a, dtype) for a in (q, k, v))
        for nw in (4, 16):
            fa.tune("attn_nw", nw)
            tag = "%s nw=%d" % (what, nw)
            # exact: as many launches as it takes for EVERY target position (the ends, both sides of every split, wave-batch and
            # unroll boundary) to have been some head's target; decoys in the stale tail and the next kv head; 3e4 behind the rows
            targets = ac.decode_targets(S, nsplit, d, plain_nw(nw, G))
            sels = ac.decode_selectors(seed, S, H, Hkv, d, targets)
            assert set(int(p) for sel in sels for p in sel.pi.ravel()) == set(targets), tag
            for sel in sels:
                assert set(sel.decoys) == ac.decode_decoy_classes(S, Hkv), (tag, sorted(sel.decoys))
                worst, ok = sel.margin()
                assert ok and worst < -ac.GAP, (tag, worst)
                got = fa.op_attention_plain(ac.as_input(sel.q.reshape(1, -1), dtype), ac.as_input(sel.k.reshape(S + G, -1), dtype),
                                            ac.as_input(sel.v.reshape(S + G, -1), dtype), S - 1, H, Hkv, d, kernel=1, nsplit=nsplit,
                                            capacity=S + G + 37, pad_value=STALE, repeat=4)
                want = sel.expected()
                for r in range(4):
                    bad = np.argwhere(got[r] != want)
                    assert bad.size == 0, "%s %s selector, launch %d: %d elements differ, first at head %d (target key %d)" % (
                        tag, dtype, r, len(bad), bad[0][1] // d, sel.pi[0, bad[0][1] // d])
            # random data against fp64; four launches on one scratch and a stale tail of 3e4 change no bit
            got = fa.op_attention_plain(qi, ki, vi, S - 1, H, Hkv, d, kernel=1, nsplit=nsplit, capacity=S + 40, repeat=4)
            ac.check_plain(got[0], ref, bound, dtype, tag, RATIOS)
            for r in range(1, 4):
                assert (got[r].view(np.uint32) == got[0].view(np.uint32)).all(), "%s %s: launch %d differs from launch 0" % (tag, dtype, r)
            pad = fa.op_attention_plain(qi, ki, vi, S - 1, H, Hkv, d, kernel=1, nsplit=nsplit, capacity=S + 40, pad_value=STALE)
            assert (pad[0].view(np.uint32) == got[0].view(np.uint32)).all(), "%s %s: the stale tail changed the output" % (tag, dtype)


# S = 100 with 64 splits: the split length rounds up to a workgroup's 16 / 32 keys, so most splits own no key (lo >= hi)
S_NSPLIT = [(S, n) for S in (1, 31, 32, 33, 255, 256, 257, 640, 1025) for n in (1, 2, 8, 9, 17, 32, 64)] + [(100, 64)]


@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("H,Hkv", [(8, 8), (28, 4), (18, 2)])             # G = 1 (parts = 8 at d = 64, 64 splits), 7, 9 = 8 + 1
@pytest.mark.parametrize("S,nsplit", S_NSPLIT)
def test_decode(fa, d, H, Hkv, S, nsplit):
    run_decode_case(fa, d, H, Hkv, S, nsplit)


@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("H,Hkv", [(12, 4), (8, 1), (24, 2), (16, 1)])    # G = 3, 8, 12 = 8 + 4, 16 = 8 + 8
@pytest.mark.parametrize("S", [33, 257, 1025])
@pytest.mark.parametrize("nsplit", [1, 2, 8, 9, 17, 32, 64])
def test_decode_other_head_layouts(fa, d, H, Hkv, S, nsplit):
    run_decode_case(fa, d, H, Hkv, S, nsplit)


PREFILL = [(2, 0, -1, 0), (33, 0, -1, 0), (100, 0, 5, 0), (64, 40, -1, 40), (70, 129, 17, 129), (70, 129, 17, 60), (40, 200, 300, 0)]


def run_prefill_case(fa, d, H, Hkv, T, s_past, window, call0, layout, kernel, dtypes):
    S, G = s_past + T, H // Hkv
    what = "prefill layout=%d kernel=%d d=%d H=%d Hkv=%d T=%d past=%d w=%d call0=%d" % (layout, kernel, d, H, Hkv, T, s_past, window, call0)
    seed = T * 3 + s_past + d + H + call0
    sel = ac.prefill_selector(seed, T, s_past, window, call0, H, Hkv, d)
    worst, ok = sel.margin()
    assert ok and worst < -ac.GAP, (what, worst)
    # (prefill_selector asserts that every decoy class the case has room for is placed)
    assert set(ac.prefill_named_targets(T, s_past, window, call0)) <= set(int(p) for p in sel.pi.ravel()), what
    want = sel.expected()
    for dtype in dtypes:
        kw = dict(layout=layout, kernel=kernel, window=window, call0=call0)
        got = fa.op_attention_plain(ac.as_input(sel.q.reshape(T, -1), dtype), ac.as_input(sel.k.reshape(S + 2 * G, -1), dtype),
                                    ac.as_input(sel.v.reshape(S + 2 * G, -1), dtype), s_past, H, Hkv, d, capacity=S + 2 * G + 37,
                                    pad_value=STALE, **kw)[0]
        bad = np.argwhere(got != want)
        assert bad.size == 0, "%s %s selector: %d elements differ, first at query %d head %d (target key %d)" % (
            what, dtype, len(bad), bad[0][0], bad[0][1] // d, sel.pi[bad[0][0], bad[0][1] // d])
        q, k, v = ac.random_case(seed, T, S, H, Hkv, d, dtype)
        qi, ki, vi = (ac.as_input(a, dtype) for a in (q, k, v))
        got = fa.op_attention_plain(qi, ki, vi, s_past, H, Hkv, d, capacity=S + 40, **kw)[0]
        if layout == 0:
            ref, bound = ac.f32_bound(q, k, v, s_past, H, Hkv, d, window, call0)
            ac.check_plain(got, ref, bound, dtype, what, RATIOS)
        else:
            check(got, reference(qi, ki, vi, s_past, H, Hkv, d, window, call0), what)
        pad = fa.op_attention_plain(qi, ki, vi, s_past, H, Hkv, d, capacity=S + 40, pad_value=STALE, **kw)[0]
        assert (pad.view(np.uint32) == got.view(np.uint32)).all(), "%s %s: the stale tail changed the output" % (what, dtype)


@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("H,Hkv", ac.LAYOUTS)
@pytest.mark.parametrize("T,s_past,window,call0", PREFILL)
def test_prefill(fa, d, H, Hkv, T, s_past, window, call0):
    run_prefill_case(fa, d, H, Hkv, T, s_past, window, call0, 0, 0, ("f32", "bf16"))


MFMA_LAYOUTS = [(8, 8), (12, 4), (28, 4), (8, 1)]


@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("H,Hkv", MFMA_LAYOUTS)
@pytest.mark.parametrize("kernel", [2, 3])
@pytest.mark.parametrize("T,s_past,window,call0", PREFILL)
def test_mfma_prefill_stale_tail_and_call0(fa, d, H, Hkv, kernel, T, s_past, window, call0):
    """the 16-row and the 32-row MFMA prefill kernels on the same cases: a chunked prefill's mask, finite stale rows behind the
    cached length (inside the last 32-key tile they are loaded and must be masked to P = 0)"""
    run_prefill_case(fa, d, H, Hkv, T, s_past, window, call0, 1, kernel, ("bf16",))


@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("H,Hkv", MFMA_LAYOUTS)
@pytest.mark.parametrize("S,nsplit", [(1, 1), (33, 1), (257, 1), (257, 2), (640, 5), (1025, 9), (100, 64)])
def test_mfma_decode_stale_tail(fa, d, H, Hkv, S, nsplit):
    G, what = H // Hkv, "mfma decode d=%d H=%d Hkv=%d S=%d nsplit=%d" % (d, H, Hkv, S, nsplit)
    seed = S * 17 + nsplit + d + H
    for sel in ac.decode_selectors(seed, S, H, Hkv, d, ac.decode_targets(S, nsplit, d, 16 if nsplit == 1 else 4, layout=1)):
        assert set(sel.decoys) == ac.decode_decoy_classes(S, Hkv), (what, sorted(sel.decoys))
        worst, ok = sel.margin()
        assert ok and worst < -ac.GAP, (what, worst)
        got = fa.op_attention_plain(ac.as_input(sel.q.reshape(1, -1), "bf16"), ac.as_input(sel.k.reshape(S + G, -1), "bf16"),
                                    ac.as_input(sel.v.reshape(S + G, -1), "bf16"), S - 1, H, Hkv, d, layout=1, kernel=1, nsplit=nsplit,
                                    capacity=S + G + 37, pad_value=STALE, repeat=4)
        want = sel.expected()
        for r in range(4):
            assert (got[r] == want).all(), "%s selector, launch %d" % (what, r)
    q, k, v = (ac.as_input(a, "bf16") for a in ac.random_case(seed, 1, S, H, Hkv, d, "bf16"))
    got = fa.op_attention_plain(q, k, v, S - 1, H, Hkv, d, layout=1, kernel=1, nsplit=nsplit, capacity=S + 40, repeat=4)
    check(got[0], reference(q, k, v, S - 1, H, Hkv, d, -1), what)
    pad = fa.op_attention_plain(q, k, v, S - 1, H, Hkv, d, layout=1, kernel=1, nsplit=nsplit, capacity=S + 40, pad_value=STALE)
    assert (pad[0].view(np.uint32) == got[0].view(np.uint32)).all(), what + ": the stale tail changed the output"
    for r in range(1, 4):
        assert (got[r].view(np.uint32) == got[0].view(np.uint32)).all(), "%s: launch %d differs from launch 0" % (what, r)
    # the existing entry point builds the same cache with zero padding: the same bits
    assert (fa.op_attention(q, k, v, S - 1, H, Hkv, d, kernel=1, nsplit=nsplit) == got[0]).all(), what + ": differs from fl_op_attention"


def test_attn_nw_selects_another_workgroup_width(fa):
    """the 16- / 8-wave forms deal the keys to the lanes differently, so on random fp32 data some output bit must differ from the
    4-wave form's: the switch the cases above rely on is alive"""
    q, k, v = ac.random_case(3, 1, 1025, 28, 4, 128, "f32")
    outs = {}
    for H, Hkv in ((28, 4), (12, 4)):                                     # eight waves (G = 7), sixteen (G = 3)
        for nw in (4, 16):
            fa.tune("attn_nw", nw)
            outs[nw] = fa.op_attention_plain(q[:, :H * 128], k, v, 1024, H, Hkv, 128, kernel=1, nsplit=1)[0]
        assert (outs[4].view(np.uint32) != outs[16].view(np.uint32)).any(), "attn_nw = 16 ran the 4-wave kernel (H = %d)" % H


def test_refused_shapes(fa):
    q, k, v = (ac.as_input(a, "bf16") for a in ac.random_case(1, 1, 4, 18, 2, 64, "bf16"))
    with pytest.raises(fa.FastLLMError):
        fa.op_attention_plain(q, k, v, 3, 18, 2, 64, layout=1)            # 9 query heads per kv head: not an MFMA shape
    fa.op_attention_plain(q, k, v, 3, 18, 2, 64, layout=0)                # ... the plain kernels take it
    with pytest.raises(fa.FastLLMError):
        fa.op_attention_plain(q, k, v, 3, 18, 2, 64, call0=4)             # call0 > s_past
