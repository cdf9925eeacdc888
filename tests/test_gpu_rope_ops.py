"""QKV projection -> RoPE -> KV append in every form, each alone against tests/rope_ref.py.
A. the stand-alone kernels (fl_op_rope_kv: scalar, vector, batch, packed): q and the WHOLE cache images bit for bit -- their slab sums,
   bias add and rotation have one rounding order (rope_ref.rotate_exact).
B. the fused epilogues (fl_op_qkv_rope: the prompt kernels by plan_qkv_rope, the single-sequence, FP8 and batched weight streams): q and
   the appended rows within rope_ref.fused_bounds, every other cache element bit-identical to the pattern it was filled with.
Rows of a multi-row input differ in magnitude by powers of two, positions differ from slots, the caches start as a recognisable
pattern and q as NaN, and every case asserts through kernels_out that it reached the kernel it names."""
import contextlib
import os

import numpy as np
import pytest

import norm_ref
import rope_ref as R
from conftest import needs_experimental

pytestmark = pytest.mark.gpu
EPS = norm_ref.EPS
HEADS = [(4, 2, 64), (2, 1, 128), (3, 1, 64), (2, 2, 128)]      # GQA, ragged head counts, MHA
# (every model's head_dim reaches the kernels padded to 64 or 128 -- weights.hip's head_pad -- so there is no other d to add for the scalar kernel)
SLABS = [1, 2, 3, 5]


@pytest.fixture(scope="module")
def fa():
    import fastllm_amd
    assert fastllm_amd.device_count() >= 1
    return fastllm_amd


@contextlib.contextmanager
def switches(fa, env=None, **tune):
    """fl_tune rows (and FL_* environment switches, re-read at once) for the block; everything back as the environment has it after"""
    saved = {k: os.environ.get(k) for k in (env or {})}
    try:
        for k, v in (env or {}).items():
            os.environ[k] = str(v)
        if env:
            fa.reload_env()
        for k, v in tune.items():
            fa.tune(k, v)
        yield
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        fa.tune("reload_env", 0)


_TABLES = {}


def tables(max_pos, d):
    if (max_pos, d) not in _TABLES:
        _TABLES[(max_pos, d)] = R.tables(max_pos, d)
    return _TABLES[(max_pos, d)]


def mix(i):
    """(n_slab, bias) of the i-th case of a loop: all eight combinations within eight cases"""
    return SLABS[i % 4], bool(((i // 4) + i) % 2)


def make_seq(count, pos, len_, sa, vt, layers, Hkv, d, dtype, seed):
    k, v = R.new_caches(layers, Hkv, sa, d, vt, dtype, seed)
    return dict(count=count, pos=pos, len=len_, seq_alloc=sa, vt=int(vt), k=k, v=v)


def rows_of(seqs):
    """(RoPE position, cache slot) of every row of the call, the sequences back to back"""
    pos = np.concatenate([s["pos"] + np.arange(s["count"]) for s in seqs])
    slot = np.concatenate([s["len"] + np.arange(s["count"]) for s in seqs])
    return pos, slot


# ==== A. the stand-alone kernels ==========================================================================================================
def exact_case(fa, form, seqs, H, Hkv, d, dtype, n_slab, bias, layers, layer, max_pos, seed, repeat=1):
    """one fl_op_rope_kv call against the exact reference: q and every sequence's whole K and V image, bit for bit.  Returns
    (kernels, q, caches)."""
    rows = sum(s["count"] for s in seqs)
    qkv, b = R.qkv_inputs(n_slab, rows, (H + 2 * Hkv) * d, seed, bias)
    cos, sin = tables(max_pos, d)
    q, caches, kernels = fa.op_rope_kv(form, qkv, cos, sin, H, Hkv, d, seqs, dtype, bias=b, layers=layers, layer=layer, repeat=repeat)
    pos, slot = rows_of(seqs)
    eq, ek, ev = R.rotate_exact(R.sum_slabs(qkv, b), cos, sin, pos, H, Hkv, d, dtype)
    msg = "form %d %s rows %d n_slab %d bias %s layer %d/%d" % (form, dtype, rows, n_slab, bias, layer, layers)
    np.testing.assert_array_equal(q, eq, err_msg=msg)
    r0 = 0
    for i, s in enumerate(seqs):
        r1 = r0 + s["count"]
        wk, wv = R.place(s["k"], s["v"], ek[r0:r1], ev[r0:r1], slot[r0:r1], s["vt"], layer)
        np.testing.assert_array_equal(caches[i][0], wk, err_msg="%s: K of sequence %d" % (msg, i))
        np.testing.assert_array_equal(caches[i][1], wv, err_msg="%s: V of sequence %d" % (msg, i))
        r0 = r1
    return kernels, q, caches


def kernel_name(fa, kernels):
    return fa.ROPE_KV_NAMES[int(kernels[0])]


@pytest.mark.parametrize("H,Hkv,d", HEADS)
@pytest.mark.parametrize("vt", [0, 1])
@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_scalar(fa, H, Hkv, d, vt, dtype):
    """rope_kv_kernel<bf16 / float>: T below the vector kernel's 16 rows, and 17 rows on the layouts it does not take (rope_vec = 0
    for bf16 with a transposed V); len 0 / 3 / up to the cache's last slot; pos != len; the second of two layers"""
    sa, max_pos, i = 24, 64, 0
    with switches(fa, rope_vec=0):
        for T in (1, 5, 17):
            for len_ in (0, 3, sa - T):
                n_slab, bias = mix(i)
                layers, layer = (2, 1) if i % 2 else (1, 0)
                seqs = [make_seq(T, len_ + 7, len_, sa, vt, layers, Hkv, d, dtype, 10 + i)]
                kernels, _, _ = exact_case(fa, 0, seqs, H, Hkv, d, dtype, n_slab, bias, layers, layer, max_pos, 1000 + i, repeat=2 if i == 0 else 1)
                assert kernel_name(fa, kernels) == "scalar" and kernels[1] == (1 if dtype == "bf16" else 0) and kernels[2] == vt, kernels
                i += 1
        # the last row of the tables: pos + T == max_pos
        seqs = [make_seq(5, max_pos - 5, 2, sa, vt, 1, Hkv, d, dtype, 50)]
        exact_case(fa, 0, seqs, H, Hkv, d, dtype, 2, True, 1, 0, max_pos, 1100)


# T: the 32-token V tile and its 8-token chunks both end ragged; len: aligned (0, 8, 24) and unaligned (5) 16-byte stores.
# (3, 1, 64) at T = 31: 31 * 4 * 4 = 496 items, not a multiple of 256
@pytest.mark.parametrize("H,Hkv,d", HEADS)
def test_vector(fa, H, Hkv, d):
    max_pos, i = 128, 0
    for T in (16, 31, 32, 33, 40, 72):
        for len_ in (0, 8, 5, 24):
            n_slab, bias = mix(i)
            layers, layer = (2, 1) if i % 3 == 1 else (1, 0)
            sa = 96 if len_ == 24 else 104                           # (24 + 72 == 96: up to the cache's last slot)
            seqs = [make_seq(T, len_ + 9, len_, sa, 1, layers, Hkv, d, "bf16", 100 + i)]
            kernels, _, _ = exact_case(fa, 0, seqs, H, Hkv, d, "bf16", n_slab, bias, layers, layer, max_pos, 2000 + i, repeat=2 if i == 0 else 1)
            assert kernel_name(fa, kernels) == "vector" and kernels[3] == (T * (H + Hkv) * (d // 16) + 255) // 256, kernels
            i += 1
    assert (31 * (3 + 1) * (64 // 16)) % 256 != 0


@pytest.mark.parametrize("H,Hkv,d", HEADS)
def test_vector_rule_falls_back_to_scalar(fa, H, Hkv, d):
    """max_seq = 100 is no multiple of 8 (the 16-byte V store could not be aligned): the scalar kernel, still exact; and f32 / a
    row-major V never take the vector kernel"""
    for T, len_ in ((33, 5), (40, 60)):
        seqs = [make_seq(T, len_ + 1, len_, 100, 1, 1, Hkv, d, "bf16", 200 + T)]
        kernels, _, _ = exact_case(fa, 0, seqs, H, Hkv, d, "bf16", 3, True, 1, 0, 128, 2100 + T)
        assert kernel_name(fa, kernels) == "scalar", kernels
    for dtype, vt in (("bf16", 0), ("f32", 1)):
        seqs = [make_seq(33, 6, 5, 104, vt, 1, Hkv, d, dtype, 210)]
        kernels, _, _ = exact_case(fa, 0, seqs, H, Hkv, d, dtype, 2, False, 1, 0, 128, 2150)
        assert kernel_name(fa, kernels) == "scalar", kernels


# the three instantiations: bf16 transposed V, bf16 row-major V, f32
@pytest.mark.parametrize("dtype,vt", [("bf16", 1), ("bf16", 0), ("f32", 0)])
@pytest.mark.parametrize("H,Hkv,d", HEADS)
def test_batch(fa, H, Hkv, d, dtype, vt):
    """rope_kv_batch_kernel<CT, VT>: every sequence its own pos, len and seq_alloc (the stride of its layer offset), layer 1 of 2"""
    allocs = (64, 40, 128, 32, 72, 48, 96, 56)
    for i, B in enumerate((1, 3, 8, 32)):
        n_slab, bias = mix(i + (4 if H == 4 else 0))
        seqs = []
        for b in range(B):
            sa = allocs[b % 8]
            len_ = (5 * b + 3) % sa if b % 4 else sa - 1                 # (every fourth: the cache's last slot)
            seqs.append(make_seq(1, (11 * b + len_ + 1) % 250, len_, sa, vt, 2, Hkv, d, dtype, 300 + b))
        kernels, _, _ = exact_case(fa, 1, seqs, H, Hkv, d, dtype, n_slab, bias, 2, 1, 256, 3000 + B, repeat=2 if B == 3 else 1)
        assert kernel_name(fa, kernels) == "batch" and kernels[1] == (1 if dtype == "bf16" else 0) and kernels[2] == vt, kernels


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
@pytest.mark.parametrize("H,Hkv,d", HEADS)
def test_packed(fa, H, Hkv, d, dtype):
    """rope_kv_packed_kernel: counts (1, 17, 5) and (33,), a member with len > 0 and pos != len, mixed value layouts and capacities in one
    pack, layer 1 of 2 -- and a member's q rows and cache are the same bytes wherever in the pack it sits"""
    def members():
        return [make_seq(1, 9, 4, 40, 1, 2, Hkv, d, dtype, 400), make_seq(17, 0, 0, 64, 0, 2, Hkv, d, dtype, 410),
                make_seq(5, 30, 27, 32, 1, 2, Hkv, d, dtype, 420)]
    N = (H + 2 * Hkv) * d
    for i, order in enumerate(((0, 1, 2), (2, 0, 1))):
        n_slab, bias = 3, True
        seqs = [members()[m] for m in order]
        # the same rows for a member in both orders: draw in member order, then permute the blocks
        qkv_m, b = R.qkv_inputs(n_slab, 23, N, 4000, bias)
        blocks = np.split(np.arange(23), [1, 18])
        perm = np.concatenate([blocks[m] for m in order])
        cos, sin = tables(64, d)
        qkv = np.ascontiguousarray(qkv_m[:, perm])
        q, caches, kernels = fa.op_rope_kv(2, qkv, cos, sin, H, Hkv, d, seqs, dtype, bias=b, layers=2, layer=1, repeat=2)
        assert kernel_name(fa, kernels) == "packed" and kernels[1] == (1 if dtype == "bf16" else 0), kernels
        pos, slot = rows_of(seqs)
        eq, ek, ev = R.rotate_exact(R.sum_slabs(qkv, b), cos, sin, pos, H, Hkv, d, dtype)
        np.testing.assert_array_equal(q, eq)
        r0, got = 0, {}
        for j, s in enumerate(seqs):
            r1 = r0 + s["count"]
            wk, wv = R.place(s["k"], s["v"], ek[r0:r1], ev[r0:r1], slot[r0:r1], s["vt"], 1)
            np.testing.assert_array_equal(caches[j][0], wk)
            np.testing.assert_array_equal(caches[j][1], wv)
            got[order[j]] = (q[r0:r1], caches[j][0], caches[j][1])
            r0 = r1
        if i == 0:
            first = got
        else:
            for m in range(3):
                for a, c in zip(first[m], got[m]):
                    np.testing.assert_array_equal(a, c, err_msg="member %d moved within the pack" % m)
    for j, (n_slab, bias) in enumerate(((1, False), (5, True))):
        seqs = [make_seq(33, 3, 7, 48, j, 2, Hkv, d, dtype, 430 + j)]
        kernels, _, _ = exact_case(fa, 2, seqs, H, Hkv, d, dtype, n_slab, bias, 2, 1, 64, 4100 + j)
        assert kernel_name(fa, kernels) == "packed", kernels


# ==== B. the fused forms =================================================================================================================
def fused_case(fa, form, T, K, H, Hkv, d, dtype, seqs, n_slab, bias, layers, layer, max_pos, seed, repeat=1, embed=None, fp8=False):
    """one fl_op_qkv_rope call against the float64 reference under the derived bound (rope_ref.fused_bounds); everything outside the
    appended slots bit-identical to the pattern; x_out bit for bit.  embed: (E, tokens) instead of x_res + delta.  Returns kernels."""
    c = R.fused_inputs(T, K, H, Hkv, d, n_slab, bias, dtype, seed)
    Wd, Wv, w_scale = c["Wd"], c["Wv"], None
    if fp8:                                                              # the reference projects with the dequantised weights
        from test_w8_abi import dequantize
        Wd, w_scale = fa.op_quantize_rows(c["Wv"])
        Wv = dequantize(Wd, w_scale)
    kw = dict(x_res=c["x"], delta=c["delta"])
    v = c["v"]
    if embed is not None:
        Ed, Ev, toks = embed
        kw, v = dict(embed=Ed, tokens=toks), Ev[toks]
    y = c["y"]
    if embed is not None or fp8:
        y = norm_ref.project(norm_ref.xs_of(v, c["w"], dtype), norm_ref.inv_rms(v), Wv, c["b"])
    cos, sin = tables(max_pos, d)
    q, caches, x_out, kernels = fa.op_qkv_rope(form, Wd, c["w"], EPS, cos, sin, H, Hkv, d, seqs, dtype, bias=c["b"], w_scale=w_scale,
                                               layers=layers, layer=layer, repeat=repeat, **kw)
    msg = "form %d %s T %d K %d heads %s n_slab %d bias %s kernels %s" % (form, dtype, T, K, (H, Hkv, d), n_slab, bias, list(kernels))
    np.testing.assert_array_equal(x_out, v, err_msg=msg)
    pos, slot = rows_of(seqs)
    (wq, wk, wv), (lq, lk, lv) = R.fused_bounds(y, cos, sin, pos, H, Hkv, d, K, dtype)
    err = np.abs(R.widen(q) - wq)
    print("%s: q worst err / bound %.3f" % (msg, float((err / lq).max())))
    assert np.isfinite(R.widen(q)).all() and (err <= lq).all(), msg
    r0 = 0
    for i, s in enumerate(seqs):
        r1 = r0 + s["count"]
        gk, gv = caches[i]
        mk, mv = R.appended_mask(s["k"], slot[r0:r1], s["vt"], layer)
        np.testing.assert_array_equal(gk[~mk], s["k"][~mk], err_msg="%s: K of sequence %d outside the appended slots" % (msg, i))
        np.testing.assert_array_equal(gv[~mv], s["v"][~mv], err_msg="%s: V of sequence %d outside the appended slots" % (msg, i))
        # the appended rows, taken out of the images in row order: [rows, Hkv d]
        ak = gk[layer][:, slot[r0:r1], :].transpose(1, 0, 2).reshape(r1 - r0, -1)
        av = (gv[layer][:, :, slot[r0:r1]].transpose(2, 0, 1) if s["vt"] else gv[layer][:, slot[r0:r1], :].transpose(1, 0, 2)).reshape(r1 - r0, -1)
        ek, ev = np.abs(R.widen(ak) - wk[r0:r1]), np.abs(R.widen(av) - wv[r0:r1])
        print("   sequence %d: k %.3f v %.3f of the bound" % (i, float((ek / lk[r0:r1]).max()), float((ev / lv[r0:r1]).max())))
        assert (ek <= lk[r0:r1]).all() and (ev <= lv[r0:r1]).all(), "%s: appended rows of sequence %d" % (msg, i)
        r0 = r1
    return kernels


def lk(fa, kernels):
    return fa.LK_NAMES[int(kernels[0])]


# ---- form 0: the prompt path ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_form0_fallback_slabs(fa, dtype):
    """the plan keeps an fp32 output (rope == 0): the plain projection, then launch_rope_kv with the bias.  bf16 at T = 33, K = 1536: the
    skinny kernel in three K slabs that rope_kv sums; the fp32 kernels never leave slabs (one)."""
    T, K, (H, Hkv, d) = 33, 1536, (2, 1, 128)
    seqs = [make_seq(T, 9, 4, 64, 1 if dtype == "bf16" else 0, 1, Hkv, d, dtype, 500)]
    kernels = fused_case(fa, 0, T, K, H, Hkv, d, dtype, seqs, 2, True, 1, 0, 64, 5000, repeat=2)
    assert kernels[3] == 0, kernels                                       # the fallback
    if dtype == "bf16":
        assert lk(fa, kernels) == "skinny" and kernels[1] == 3, kernels
    else:
        assert lk(fa, kernels) == "f32_rows" and kernels[1] == 1, kernels


# T = 130: a ragged second row tile; K = 256: four K tiles, so 1, 2 and 4 slices; N = 512 from two head shapes, N = 320 = a ragged column
# tile; h4_split = 3 must be planned as 2 (a 128-wide head's halves need one owner)
@pytest.mark.parametrize("H,Hkv,d", [(4, 2, 64), (2, 1, 128), (3, 1, 64)])
@pytest.mark.parametrize("split", [1, 2, 3, 4])
def test_form0_h4(fa, H, Hkv, d, split):
    T, K = 130, 256
    with switches(fa, gemm_h4=2, h4_split=split):
        for vt in (0, 1):
            bias = bool((split + vt) % 2)
            seqs = [make_seq(T, 8, 5, 160, vt, 2, Hkv, d, "bf16", 510 + vt)]
            kernels = fused_case(fa, 0, T, K, H, Hkv, d, "bf16", seqs, 2, bias, 2, 1, 160, 5100 + split, repeat=2)
            assert lk(fa, kernels) == "h4" and kernels[1] == (2 if split == 3 else split) and kernels[3] == 1, kernels


# The smallest T >= 768 with a ragged last row tile that plan_qkv_rope puts on the four-wave kernel with gemm_h4 = 0 is T = 769 (three
# whole row tiles and one row), at N = 9472 columns: found by asking the planner for every T in 769 .. 3000 that is no multiple of 256 and
# every N = 2048 .. 16384 in steps of 128 and taking the smallest T * N it answers LK_4W_ROPE for -- the kernel is only planned where
# ONE plain grid of 256 x 256 tiles beats K slabs, i.e. from about 130 tiles on (4 x 37 = 148 here).  FL_GEMM_4W = 2 lifts the rule's
# K >= 3072 (gemm_4w_rule), which keeps the float64 reference at 7.5 GFLOP with K = 512.  N = 9472 is 148 heads of 64 or 74 of 128.
@pytest.mark.parametrize("H,Hkv,d", [(140, 4, 64), (70, 2, 128)])
def test_form0_4w_rope(fa, H, Hkv, d):
    T, K = 769, 512
    with switches(fa, {"FL_GEMM_4W": 2}, gemm_h4=0):
        seqs = [make_seq(T, 6, 3, 800, 1, 1, Hkv, d, "bf16", 520)]
        kernels = fused_case(fa, 0, T, K, H, Hkv, d, "bf16", seqs, 1, d == 64, 1, 0, 800, 5200)
    assert lk(fa, kernels) == "4w_rope" and fa.LK_NAMES[int(kernels[2])] == "none" and kernels[3] == 1, kernels


def test_form0_4w_rope_with_a_peeled_h4_tail(fa):
    """4096 x 4736 x 1024: 16 x 19 tiles of 256 x 256 -- one whole round (16 column tiles) on the four-wave kernel, the last 640 columns
    (q heads 64 .. 69, both k heads, both v heads) on the 128 x 256 kernel in two K slices with col_base = 4096.  Peeling starts at a
    full round of the chip and K >= 1024 (gemm_peel_plan), so this is the smallest such plan: 40 GFLOP of float64 reference."""
    T, K, (H, Hkv, d) = 4096, 1024, (70, 2, 64)
    with switches(fa, {"FL_GEMM_4W": 2}):
        seqs = [make_seq(T, 2, 0, T, 1, 1, Hkv, d, "bf16", 530)]
        kernels = fused_case(fa, 0, T, K, H, Hkv, d, "bf16", seqs, 1, True, 1, 0, T + 8, 5300)
    assert lk(fa, kernels) == "4w_rope" and fa.LK_NAMES[int(kernels[2])] == "h4" and kernels[3] == 1, kernels


@needs_experimental
@pytest.mark.parametrize("T", [5, 33, 100])
@pytest.mark.parametrize("H,Hkv,d", [(4, 2, 64), (2, 1, 128)])
def test_form0_skf(fa, T, H, Hkv, d):
    """the short-prompt GEMM's RoPE epilogue (N = 512: whole 128-column strips)"""
    with switches(fa, gemm_skf=2):
        for vt in (0, 1):
            seqs = [make_seq(T, 8, 5, 128, vt, 2, Hkv, d, "bf16", 540 + vt)]
            kernels = fused_case(fa, 0, T, 256, H, Hkv, d, "bf16", seqs, 2, bool(vt), 2, 1, 128, 5400 + T, repeat=2)
            assert lk(fa, kernels) == "skf" and kernels[3] == 1, kernels


# ---- forms 1 and 2: the single-sequence weight streams --------------------------------------------------------------------------------------
def _embedding(K, dtype, seed):
    rs = np.random.RandomState(seed)
    V = 7
    E = (rs.standard_normal((V, K)) * np.float32(2.0) ** np.arange(V)[:, None]).astype(np.float32)       # every row another magnitude
    Ed, Ev = norm_ref.as_dtype(E, dtype)
    return Ed, Ev


@pytest.mark.parametrize("form,dtype", [(1, "bf16"), (1, "f32"), (2, "bf16")])
@pytest.mark.parametrize("K", [256, 1536])
@pytest.mark.parametrize("H,Hkv,d", HEADS)
def test_gemv_streams(fa, form, dtype, K, H, Hkv, d):
    """launch_gemv / launch_gemv_w8 with EPI_QKV_ROPE and the norm prologue: both value layouts (v_ld 0 and seq_alloc), bias on / off,
    residual + delta and embedding-row input, the second of two layers"""
    i = 0
    for vt in (0, 1):
        for bias in (False, True):
            n_slab = (0, 1)[i % 2] if form == 2 else (0, 1, 3, 2)[i % 4]
            seqs = [make_seq(1, 37 + i, 11 + i, 48, vt, 2, Hkv, d, dtype, 600 + i)]
            kernels = fused_case(fa, form, 1, K, H, Hkv, d, dtype, seqs, n_slab, bias, 2, 1, 64, 6000 + K + i, repeat=2, fp8=form == 2)
            assert lk(fa, kernels) == "gemv" and kernels[3] == 1, kernels
            i += 1
    Ed, Ev = _embedding(K, dtype, 61)
    seqs = [make_seq(1, 63, 47, 48, 1, 1, Hkv, d, dtype, 610)]          # the tables' last row, the cache's last slot
    fused_case(fa, form, 1, K, H, Hkv, d, dtype, seqs, 0, True, 1, 0, 64, 6100 + K, repeat=2, embed=(Ed, Ev, [5]), fp8=form == 2)


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_gemv_ragged_last_row_group(fa, dtype):
    """gemv_row_of<EPI_QKV_ROPE>: with four rows (two pairs) per group -- gemv_r = 4 -- and 15 pairs (five heads of 6) the last group holds
    one pair and one pair past N, which must not be stored.  (With head_dim 64 / 128 the pair count is even and no group is ragged; the FP8
    stream has two rows per group and no ragged group at all.)"""
    H, Hkv, d, K = 3, 1, 6, 256
    with switches(fa, gemv_r=4, gemv_u=2):
        for vt in (0, 1):
            seqs = [make_seq(1, 9, 4, 16, vt, 1, Hkv, d, dtype, 620 + vt)]
            fused_case(fa, 1, 1, K, H, Hkv, d, dtype, seqs, 1, True, 1, 0, 16, 6200, repeat=2)


# ---- form 3: the batched stream --------------------------------------------------------------------------------------------------------------
# valu: the VALU kernels (gemv_parts.h's row map and store); default: the MFMA forms from three streams on (their own copy of both)
@pytest.mark.parametrize("mode", ["valu", "default"])
@pytest.mark.parametrize("K", [256, 1536])
@pytest.mark.parametrize("H,Hkv,d", HEADS)
def test_gemv_batch(fa, mode, K, H, Hkv, d):
    allocs = (64, 32, 128, 96, 160, 32, 64, 224)
    with switches(fa, **({"batch_mfma_min": 9} if mode == "valu" else {})):
        for i, B in enumerate((1, 3, 8)):
            for bias in (False, True):
                n_slab = (1, 3)[(i + bias) % 2]
                seqs = []
                for b in range(B):
                    sa = allocs[b]
                    len_ = (7 * b + 2) % sa if b != 1 else sa - 1
                    seqs.append(make_seq(1, (13 * b + len_ + 3) % 250, len_, sa, 1, 2, Hkv, d, "bf16", 700 + b))
                kernels = fused_case(fa, 3, B, K, H, Hkv, d, "bf16", seqs, n_slab, bias, 2, 1, 256, 7000 + B + K, repeat=2)
                assert lk(fa, kernels) == "gemv" and kernels[1] == 1 and kernels[3] == 1, kernels
    Ed, Ev = _embedding(K, "bf16", 71)
    seqs = [make_seq(1, 3 + b, b, 32, 1, 1, Hkv, d, "bf16", 710 + b) for b in range(5)]
    with switches(fa, **({"batch_mfma_min": 9} if mode == "valu" else {})):
        fused_case(fa, 3, 5, K, H, Hkv, d, "bf16", seqs, 0, True, 1, 0, 64, 7100 + K, embed=(Ed, Ev, [6, 2, 5, 2, 4]))
