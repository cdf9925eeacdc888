"""attn_oproj_rep_kernel (k_attn_rep.hip) ALONE -- the launch every default bf16 model takes for decode steps on short caches --
through fl_op_attn_oproj_rep, which builds the cache in the model's layout and calls launch_attn_oproj_rep as the decode step does.
test_gpu_attn_rep.py sees this kernel only through whole-model logits at the bf16 model tolerance, at four head layouts, one tile
or two per slice and N <= 2048.

Cases, reference, emulation and bound are attn_rep_ref.py's (checked without a GPU by test_attn_rep_ref.py).  Per (head size, head
layout, S):
  * exact: the decode selectors of the case -- every target key (key 0, key S - 1, both sides of every tile edge through the third
    burst, every slice's first key in the first and the second burst) is some head's target in one of them, decoys sit in the stale
    tail and in the next kv head, 3e4 behind the rows -- each with the signed selection matrix and with the small-integer W_o / V:
    four launches, each bit for bit what the indices say.  The selectors and the row counts N of the layout are dealt round robin
    (selector i with N[i % len]) until both lists are through: every selector and every N runs in both forms in every case, and over
    the S list every N meets every kind of target.  A mismatch names the row, the W_o column, the head and its target key;
  * random (attn_cases.random_case, W_o N(0, 1) in bf16) at every N of the layout: inside the derived bound, four launches
    bit-identical, a stale tail of 3e4 instead of 0 changes no bit.
Head layouts: G = 1, 3, 4, 5, 8; nslice = 1, 2, 4, 8; K / 8 = 32 ... 256 (idle lanes, a ragged last 64-chunk group, all four).  N:
1, 7, 9, K and -- at two layouts per head size, one per GMAX -- 2048, 2049, 2048 + 17, 4096 (two rows per wave, odd N).  The S list
runs bursts the model's capacity rule never reaches (FL_ATTN_REP=2 and the profiles do); the largest S the rule allows is the last
case of a layout, and info[0] is checked against the rule on every call."""
import numpy as np
import pytest

import attn_cases as ac
import attn_rep_ref as ar
import synth

pytestmark = pytest.mark.gpu

RATIOS = {}                    # d -> [(err / bound, case)]
RAN = set()                    # (d, GMAX, rows per wave) of every launch


@pytest.fixture(scope="module")
def fa():
    import fastllm_amd
    assert fastllm_amd.device_count() >= 1
    yield fastllm_amd
    for d, rows in sorted(RATIOS.items()):
        print("attn_oproj_rep d=%d: largest err / bound %.4f (%s) over %d checks" % ((d,) + max(rows) + (len(rows),)))
    print("attn_oproj_rep instantiations run (d, GMAX, rows per wave): %s" % sorted(RAN))


def bits(a):
    return synth.f32_to_bf16_bits(np.ascontiguousarray(a, dtype=np.float32))


def launch(fa, q, k, v, w, S, H, Hkv, d, cap, N, **kw):
    """one op call; records the instantiation and checks info against the shape"""
    out, info = fa.op_attn_oproj_rep(bits(q).reshape(-1), bits(k).reshape(k.shape[0], -1), bits(v).reshape(v.shape[0], -1), w, S - 1, H, Hkv, d,
                                     capacity=cap, **kw)
    G = H // Hkv
    assert list(info) == [int(ar.model_rule_case(S, cap, Hkv, d)), 1, ar.rpw(N), 4 if G <= 4 else 8, -(-N // (8 * ar.rpw(N))), ar.nslice(Hkv)], list(info)
    RAN.add((d, int(info[3]), int(info[2])))
    return out


def check_random(got, ref, B, d, what):
    assert np.isfinite(got).all(), what + ": non-finite output (a row the kernel did not write?)"
    err = np.abs(got.astype(np.float64) - ref)
    ratio = float((err / B).max())
    RATIOS.setdefault(d, []).append((ratio, what))
    print("%s: max err %.3g, worst err / bound %.4f" % (what, err.max(), ratio))
    assert ratio <= 1.0, "%s: err / bound %.3f at row %d (err %.3g)" % (what, ratio, int((err / B).argmax()), err.max())


def run_exact(fa, d, H, Hkv, S, cap, Ns, seed):
    G, what = H // Hkv, "d=%d H=%d Hkv=%d S=%d" % (d, H, Hkv, S)
    sels = ar.selectors(seed, S, H, Hkv, d)
    assert set(int(p) for sel in sels for p in sel.pi.ravel()) == set(ar.targets(S, Hkv, d)), what
    for i in range(max(len(sels), len(Ns))):
        sel, N = sels[i % len(sels)], Ns[i % len(Ns)]
        for name, v, w, want, where in ar.exact_forms(sel, N, i if N * H * d <= 1 << 20 else N):
            out = launch(fa, sel.q, sel.k, v, bits(w), S, H, Hkv, d, cap, N, pad_value=ar.STALE, repeat=4)
            for r in range(4):
                bad = ar.first_difference(out[r], want)
                assert bad is None, "%s N=%d %s, selector %d, launch %d: row %d is %r, not %r (%s)" % (
                    what, N, name, i % len(sels), r, bad, out[r][bad], want[bad], where(bad))


def run_random(fa, d, H, Hkv, S, cap, Ns):
    what = "d=%d H=%d Hkv=%d S=%d" % (d, H, Hkv, S)
    q, k, v = ar.random_inputs(d, H, Hkv, S)
    wf = ar.random_w(d, H, Hkv)
    ref, B, _, _ = ar.bound(q, k, v, wf[:max(Ns)], S, H, Hkv, d)
    wb = bits(wf)
    for N in Ns:
        out = launch(fa, q, k, v, wb[:N], S, H, Hkv, d, cap, N, repeat=4)
        check_random(out[0], ref[:N], B[:N], d, "%s N=%d" % (what, N))
        for r in range(1, 4):
            assert (out[r].view(np.uint32) == out[0].view(np.uint32)).all(), "%s N=%d: launch %d differs from launch 0" % (what, N, r)
        pad = launch(fa, q, k, v, wb[:N], S, H, Hkv, d, cap, N, pad_value=ar.STALE)
        assert (pad[0].view(np.uint32) == out[0].view(np.uint32)).all(), "%s N=%d: the stale tail changed the output" % (what, N)


CASES = [(d, H, Hkv, S, cap) for d in (64, 128) for H, Hkv in ar.layouts(d) for S, cap in ar.s_cases(H, Hkv, d)]


@pytest.mark.parametrize("d,H,Hkv,S,cap", CASES)
def test_attn_oproj_rep(fa, d, H, Hkv, S, cap):
    Ns = ar.n_list(d, H, Hkv)
    run_exact(fa, d, H, Hkv, S, cap, Ns, ar.random_seed(d, H, Hkv, S))
    run_random(fa, d, H, Hkv, S, cap, Ns)


def test_all_eight_instantiations_run(fa):
    """<D 64 / 128, GMAX 4 / 8, RPW 1 / 2>: one small case each (and whatever the cases above ran); the set reported by the op has
    all eight members"""
    ran = set()
    for d in (64, 128):
        for H, Hkv in ar.LARGE_N[d]:
            for N in (9, 2049):
                before = set(RAN)
                RAN.clear()
                run_random(fa, d, H, Hkv, 33, 33 + H // Hkv + 37, [N])
                ran |= RAN
                RAN.update(before)
    assert ran == {(d, g, r) for d in (64, 128) for g in (4, 8) for r in (1, 2)}, sorted(ran)


@pytest.mark.parametrize("d,H,Hkv,S", [(64, 32, 4, 300), (128, 12, 4, 129), (64, 5, 1, 257)])
def test_agrees_with_the_decode_attention_launch(fa, d, H, Hkv, S):
    """x of the MFMA decode kernel (fl_op_attention, one split) through an fp64 W_o: the two kernels merge their partial results in
    another order and may round x differently by one bf16 ulp (2^-8 |x|); beyond that only this kernel's dot product is left"""
    K = H * d
    q, k, v = ar.random_inputs(d, H, Hkv, S)
    w = ar.random_w(d, H, Hkv)[:K]
    x = fa.op_attention(bits(q), bits(k), bits(v), S - 1, H, Hkv, d, kernel=1, nsplit=1)[0].astype(np.float64)
    out = launch(fa, q, k, v, bits(w), S, H, Hkv, d, S + H // Hkv + 37, K)[0]
    W = w.astype(np.float64)
    lim = ar.dot_bound(w, x, K) + 2.0 ** -8 * (np.abs(W) @ np.abs(x))
    err = np.abs(out.astype(np.float64) - W @ x)
    print("d=%d H=%d Hkv=%d S=%d vs fl_op_attention: worst err / bound %.4f" % (d, H, Hkv, S, (err / lim).max()))
    assert (err <= lim).all(), (err / lim).max()


def test_the_model_takes_this_launch_where_the_rule_says_so(fa):
    """the rule table of test_attn_rep_abi.py and the model agree: a TinyLlama-width model with a cache of 96 positions runs
    attn_oproj[rep..., and the op reports the model's rule as met for that shape (and not for a cache of 128)"""
    from fastllm_amd.configs import MODEL_CONFIGS
    from test_gpu_fullsize import pooled_weights
    cfg = dict(MODEL_CONFIGS["tinyllama-1.1b"], num_hidden_layers=4)
    H, Hkv, h = cfg["num_attention_heads"], cfg["num_key_value_heads"], cfg["hidden_size"]
    gm = fa.Model(cfg, pooled_weights(cfg), dtype="bf16")
    c = gm.new_cache(96)
    ids = synth.prompt_ids(cfg, 12, seed=3)
    gm.forward(c, ids[:11], 0)
    gm.profile_begin()
    gm.forward(c, ids[11:12], 11)
    names = [s["name"] for s in gm.profile_end()]
    gm.close()
    assert any(n.startswith("attn_oproj[rep") for n in names), names
    assert fa.op_attn_oproj_rep_info(H, Hkv, h // H, h, 96)[0] == 1
    assert fa.op_attn_oproj_rep_info(H, Hkv, h // H, h, 128)[0] == 0


def test_refused_calls(fa):
    q, k, v = ar.random_inputs(64, 9, 1, 4)
    w = bits(np.zeros((8, 9 * 64), np.float32))
    with pytest.raises(fa.FastLLMError):
        fa.op_attn_oproj_rep(bits(q).reshape(-1), bits(k), bits(v), w, 3, 9, 1, 64)                # 9 query heads per kv head
    q, k, v = ar.random_inputs(64, 8, 8, 4)
    w = bits(np.zeros((8, 8 * 64), np.float32))
    with pytest.raises(fa.FastLLMError):
        fa.op_attn_oproj_rep(bits(q).reshape(-1), bits(k), bits(v), w, 3, 8, 8, 64, capacity=33 * 32)   # 33 tiles in the one slice
    with pytest.raises(fa.FastLLMError):
        fa.op_attn_oproj_rep(bits(q).reshape(-1), bits(k), bits(v), w, 4, 8, 8, 64)                # S = 5 > 4 rows
