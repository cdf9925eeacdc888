"""tests/encoder_ops_ref.py checked on the CPU, at the shapes tests/test_gpu_encoder_ops.py uses: the exact parts keep the kernels'
association, the derived LayerNorm and GELU bounds hold for a float32 restatement of the kernels with room to spare (<= 0.5 x the
bound) and are missed by planted errors (> 4 x the bound on the rows made for them), and the two GELU forms are more than 20 bounds
apart.  Every figure is printed (pytest -s)."""
import numpy as np
import pytest

import bert_ref
import decoder_ref
import encoder_ops_ref as R

# which rows (by kind) each planted error must show on
PLANTED = (("hm1", (0, 3)), ("onepass", (2,)), ("eps", (3, 4)))


def test_exact_parts_keep_the_kernels_association():
    """the slabs and the bias are summed first (in slab order), then added to x: with 2^24, 1, -2^24 every other order shows"""
    big = np.float32(2.0 ** 24)
    slabs = np.array([[[big]], [[1.0]], [[-big]]], np.float32)
    assert R.slab_sum(slabs, None)[0, 0] == 0.0 and R.slab_sum(slabs[[0, 2, 1]], None)[0, 0] == 1.0
    assert R.slab_sum(slabs, np.array([0.5], np.float32))[0, 0] == 0.5
    c = dict(x=np.array([[1.0]], np.float32), slabs=np.array([[[big]], [[-big]]], np.float32), bias=None)
    assert R.add_ln_prenorm(c)[0, 0] == 1.0                  # x + (d0 + d1); (x + d0) + d1 would give 0
    c = R.embed_case(9, 8, "bf16")
    p = np.array([0, 0, 1, 2, 0, 1, 0, 1, 2])                # the positions of the ragged batch [1, 3, 2, 3]
    want = (c["word"][c["ids"]] + c["pos"][p]) + c["tt0"]
    assert R.same_bits(R.embed_prenorm(c, True), want) and len(set(c["ids"])) == 9
    # the pooled means: row order from +0, one divide
    x = np.array([[big], [1.0], [-big], [3.0]], np.float32)
    assert R.pool_means(x, [3, 1]).tolist() == [[0.0], [3.0]]


def test_rows_have_their_kinds_and_none_is_constant():
    for T, h in R.LN_SHAPES:
        for v in (R.add_ln_prenorm(R.add_ln_case(T, h, 3, True)), R.embed_prenorm(R.embed_case(T, h, "bf16"), False),
                  R.embed_prenorm(R.embed_case(T, h, "f32"), True)):
            assert v.shape == (T, h) and (v.std(axis=1) > 0).all()
        v = R.add_ln_prenorm(R.add_ln_case(T, h, 3, True)).astype(np.float64)
        if h >= 512:
            for t in range(min(T, 5)):
                mean, std = R.KINDS[t]
                assert abs(v[t].mean() - mean) <= 0.2 * std and 0.8 * std <= v[t].std() <= 1.2 * std, (T, h, t)
    v = R.add_ln_prenorm(R.add_ln_case(9, 768, 1, False)).astype(np.float64)       # rows 0 and 5 are of one kind, a power of two apart
    assert max(v[5].std() / v[0].std(), v[0].std() / v[5].std()) > 1.5


def _ln_cases(T, h):
    """(name, pre-norm rows, w, b) of the GPU test's LayerNorm inputs at one shape"""
    out = []
    for n_slab, bias in ((1, False), (4, True)):
        c = R.add_ln_case(T, h, n_slab, bias)
        out.append(("add_ln slabs %d bias %d" % (n_slab, bias), R.add_ln_prenorm(c), c["w"], c["b"]))
    for dtype in ("f32", "bf16"):
        c = R.embed_case(T, h, dtype)
        for tt in (False, True):
            out.append(("embed %s tt0 %d" % (dtype, tt), R.embed_prenorm(c, tt), c["w"], c["b"]))
    return out


@pytest.mark.parametrize("eps", R.EPS)
@pytest.mark.parametrize("T,h", R.LN_SHAPES)
def test_layernorm_bound_holds_for_the_restatement_and_not_for_planted_errors(T, h, eps):
    onepass = []
    for name, v, w, b in _ln_cases(T, h):
        o, lim = R.ln_bound(v, w, b, eps)
        assert np.isfinite(o).all() and (lim > 0).all()
        room = max(R.worst(R.ln_restate(v, w, b, eps, fused) - o, lim) for fused in (False, True))
        line = "T=%d h=%d eps=%g %s: restatement %.3f" % (T, h, eps, name, room)
        assert room <= 0.5, line
        # The planted errors, on the rows as written (fp32 inputs; token-type row off: it is an N(0, 0.5^2) row of its own).  bf16
        # tables round the word rows, so their statistics are the kinds' only nominally: figures printed, not asserted.
        exact_kinds = not name.startswith("embed bf16") and not name.endswith("tt0 1")
        for what, kinds in PLANTED:
            bad = np.abs(R.ln_planted(v, w, b, eps, what) - o) / lim
            for t in range(min(T, len(R.KINDS))):
                if R.row_kind(t) in kinds:
                    line += "; %s row %d %.1f" % (what, t, bad[t].max())
                    if exact_kinds and what == "onepass":
                        onepass.append(bad[t].max())
                    elif exact_kinds:
                        assert bad[t].max() > 4.0, line
        print(line)
    # The one-pass variance errs by ROUNDING (a few quanta of 2^-4 on a variance of 1), so on eight values it can come out right by
    # luck in one input: it must show in the inputs of this shape taken together, as a kernel has to pass all of them.
    if onepass:
        assert max(onepass) > 4.0 and (h < 512 or min(onepass) > 4.0), onepass


@pytest.mark.parametrize("T,h", R.LN_SHAPES)
def test_token_type_row_moves_every_row_by_more_than_six_bounds(T, h):
    """the GPU test asserts that the results with and without the token-type row are more than 4 bounds apart in every row; each lies
    within one bound of its reference, so the references must be more than 6 apart"""
    for dtype in ("f32", "bf16"):
        c = R.embed_case(T, h, dtype)
        for eps in R.EPS:
            (o0, l0), (o1, l1) = (R.ln_bound(R.embed_prenorm(c, tt), c["w"], c["b"], eps) for tt in (False, True))
            apart = (np.abs(o1 - o0) / np.maximum(l0, l1)).max(axis=1)
            assert (apart > 6.0).all(), (T, h, dtype, eps, apart)


def test_layernorm_reference_is_bert_refs():
    c = R.add_ln_case(9, 520, 2, True)
    v = R.add_ln_prenorm(c).astype(np.float64)
    np.testing.assert_allclose(R.ln_ref(v, c["w"], c["b"], 1e-5)[0], bert_ref.layer_norm(v, c["w"].astype(np.float64), c["b"].astype(np.float64), 1e-5),
                               rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("T,N", R.ACT_SHAPES)
def test_gelu_bound_holds_for_float32_and_separates_the_two_forms(T, N):
    for n_slab, bias in ((1, False), (3, True)):
        c = R.act_case(T, N, n_slab, bias)
        v = R.slab_sum(c["slabs"], c["bias"])
        assert np.abs(v).max() <= 16 and len(np.unique(v)) > v.size // 2
        if bias:
            assert len(np.unique(c["bias"])) == N and np.abs(c["bias"]).max() > 0.5       # a bias from the wrong column is gross
        ref = {}
        for act in ("gelu_tanh", "gelu_erf"):
            g, lim = R.gelu_bound(v, act, "f32")
            y = R.gelu32(v, act)
            room = R.worst(y - g, lim)
            gb, limb = R.gelu_bound(v, act, "bf16")
            roomb = R.worst(R.widen(R.as_stored(y, "bf16")) - gb, limb)
            print("T=%d N=%d slabs %d bias %d %s: float32 %.3f of the bound, rounded to bf16 %.3f" % (T, N, n_slab, bias, act, room, roomb))
            assert room <= 0.5 and roomb <= 1.0
            np.testing.assert_allclose(g, bert_ref.gelu(v.astype(np.float64), act), rtol=1e-13, atol=0)
            ref[act] = (g, lim)
        gap = R.worst(ref["gelu_tanh"][0] - ref["gelu_erf"][0], np.maximum(ref["gelu_tanh"][1], ref["gelu_erf"][1]))
        print("    the two forms are %.0f bounds apart at their worst point" % gap)
        assert gap >= 20.0                                   # a swapped option cannot pass in fp32


def test_a_quarter_bf16_ulp_cannot_be_met():
    """2^-9 |g| is not a bound on round-to-nearest-even: the correctly rounded float64 reference itself exceeds it on a good part of
    the inputs, while half an ulp of g is never exceeded."""
    v = R.slab_sum(R.act_case(5, 1536, 1, False)["slabs"], None)
    g = R.gelu64(v, "gelu_erf")
    g = g[np.abs(g) > 1e-30]
    err = np.abs(R.widen(R.as_stored(g.astype(np.float32), "bf16")) - g.astype(np.float32))
    assert (err <= R.rope_ref.half_ulp_bf16(g.astype(np.float32))).all()
    assert (err > 2.0 ** -9 * np.abs(g)).mean() > 0.05


@pytest.mark.parametrize("h", R.POOL_H)
def test_pooling_reference(h):
    for lengths in R.POOL_LENGTHS:
        x = R.pool_case(lengths, h)
        m = R.pool_means(x, lengths)
        off = np.concatenate([[0], np.cumsum(lengths)])
        for s, n in enumerate(lengths):
            exact = x[off[s]:off[s + 1]].astype(np.float64).mean(axis=0)
            assert (np.abs(m[s] - exact) <= (n + 1) * R.U * np.abs(x[off[s]:off[s + 1]].astype(np.float64)).sum(axis=0) / n).all()
        # a float32 normalisation of the exact means passes decoder_ref.check_normalized; a member that takes a neighbour's row does not
        nrm = np.sqrt((m * m).sum(axis=1, keepdims=True, dtype=np.float32))
        decoder_ref.check_normalized(m / nrm, m, "float32 normalisation")
        assert np.abs(np.linalg.norm((m / nrm).astype(np.float64), axis=1) - 1.0).max() <= 1e-5
        if len(lengths) > 1:
            shifted = R.pool_means(x, [lengths[0] + 1, lengths[1] - 1] + list(lengths[2:]))
            with pytest.raises(AssertionError):
                decoder_ref.check_normalized(decoder_ref.normalize_f64(shifted).astype(np.float32), m, "a row of the neighbour")
