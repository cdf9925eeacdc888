"""The encoder's row kernels ALONE (fl_op_encoder_rows: launch_encoder_embed_ln, launch_encoder_add_ln, launch_encoder_bias_act,
launch_encoder_pool_l2) against tests/encoder_ops_ref.py, at the widths where a lane or a thread takes a second trip, with split-K slabs,
and on rows whose statistics a subtly wrong LayerNorm does not survive.

* what is exact is compared bit for bit: xn against the returned residual row (two stores of one register; RNE in bf16), the slab +
  bias sum of bias_act with act = none, and the neighbours' independence of a pooled member;
* LayerNorm and GELU outputs are compared with float64 of the exact fp32 pre-norm / pre-activation values, within the bounds derived
  in encoder_ops_ref.py (ln_bound, gelu_bound) -- tests/test_encoder_ops_ref.py shows on the CPU that a float32 restatement uses at
  most half of them and that an h - 1 divisor, a one-pass variance, the wrong eps and the other GELU form miss them by far;
* the pooled rows against decoder_ref.check_normalized on the exact float32 means.
Every LayerNorm and GELU case prints its achieved error / bound (pytest -s); the worst per form is printed at the end."""
import functools

import numpy as np
import pytest

import decoder_ref
import encoder_ops_ref as R

pytestmark = pytest.mark.gpu

DTYPES = ("f32", "bf16")
_WORST = {}


@pytest.fixture(scope="module")
def fa():
    import fastllm_amd
    assert fastllm_amd.device_count() >= 1
    yield fastllm_amd
    print("\nworst achieved error / bound per form: " + ", ".join("%s %.3f" % kv for kv in sorted(_WORST.items())))


def _frozen(c):
    for a in c.values() if isinstance(c, dict) else [c]:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return c


embed_case = functools.lru_cache(maxsize=None)(lambda T, h, dtype: _frozen(R.embed_case(T, h, dtype)))
add_ln_case = functools.lru_cache(maxsize=None)(lambda T, h, n_slab, bias: _frozen(R.add_ln_case(T, h, n_slab, bias)))
act_case = functools.lru_cache(maxsize=None)(lambda T, N, n_slab, bias: _frozen(R.act_case(T, N, n_slab, bias)))
pool_case = functools.lru_cache(maxsize=None)(lambda lengths, h: _frozen(R.pool_case(list(lengths), h)))


def check_ln(form, what, x_res, xn, v, w, b, eps, dtype):
    """the residual rows within ln_bound of the float64 LayerNorm of the exact pre-norm rows v; xn the same register as stored"""
    o, lim = R.ln_bound(v, w, b, eps)
    assert x_res.dtype == np.float32 and x_res.shape == v.shape and np.isfinite(x_res).all(), what     # (an unwritten element is NaN)
    assert np.isfinite(R.widen(xn)).all(), what
    assert R.same_bits(xn, R.as_stored(x_res, dtype)), what
    room = R.worst(x_res - o, lim)
    _WORST[form] = max(_WORST.get(form, 0.0), room)
    print("\n%s: error / bound %.3f" % (what, room), end="")
    assert room <= 1.0, (what, room)
    return o, lim


# ---- embedding sum + LayerNorm --------------------------------------------------------------------------------------------------------
def run_embed(fa, c, with_tt0, eps, repeat=1):
    return fa.op_encoder_embed_ln(c["word_bits"], c["pos_bits"], c["ids"], c["lengths"], c["w"], c["b"], eps, c["dtype"],
                                  tt0=c["tt0_bits"] if with_tt0 else None, repeat=repeat)


@pytest.mark.parametrize("eps", R.EPS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("T,h", R.LN_SHAPES)
def test_embed_ln(fa, T, h, dtype, eps):
    c = embed_case(T, h, dtype)
    got = {}
    for tt in (False, True):
        x_res, xn = run_embed(fa, c, tt, eps)
        o, lim = check_ln("embed_ln", "embed_ln T=%d h=%d %s eps=%g tt0=%d" % (T, h, dtype, eps, tt), x_res, xn, R.embed_prenorm(c, tt), c["w"], c["b"], eps, dtype)
        got[tt] = (x_res, lim)
    # the token-type row bites: in every row the two results are more than 4 bounds apart, so neither passes as the other
    apart = (np.abs(got[True][0].astype(np.float64) - got[False][0]) / np.maximum(got[True][1], got[False][1])).max(axis=1)
    assert (apart > 4.0).all(), apart


# ---- residual add + LayerNorm ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("T,h", R.LN_SHAPES)
def test_add_ln(fa, T, h, dtype):
    for n_slab in (1, 2, 3, 4):
        for bias in (False, True):
            c = add_ln_case(T, h, n_slab, bias)
            for eps in R.EPS:
                x_res, xn = fa.op_encoder_add_ln(c["x"], c["slabs"], c["w"], c["b"], eps, dtype, bias=c["bias"])
                check_ln("add_ln", "add_ln T=%d h=%d %s slabs %d bias %d eps=%g" % (T, h, dtype, n_slab, bias, eps), x_res, xn, R.add_ln_prenorm(c),
                         c["w"], c["b"], eps, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_layernorm_launches_repeat_bit_for_bit(fa, dtype):
    """repeat = 3: the call itself fails if a launch gives other bytes than the first; the result is the single launch's"""
    c = embed_case(9, 1032, dtype)
    one, three = run_embed(fa, c, True, 1e-12), run_embed(fa, c, True, 1e-12, repeat=3)
    assert R.same_bits(one[0], three[0]) and R.same_bits(one[1], three[1])
    c = add_ln_case(9, 1032, 3, True)
    one = fa.op_encoder_add_ln(c["x"], c["slabs"], c["w"], c["b"], 1e-5, dtype, bias=c["bias"])
    three = fa.op_encoder_add_ln(c["x"], c["slabs"], c["w"], c["b"], 1e-5, dtype, bias=c["bias"], repeat=3)
    assert R.same_bits(one[0], three[0]) and R.same_bits(one[1], three[1])


# ---- bias + GELU --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("T,N", R.ACT_SHAPES)
def test_bias_act(fa, T, N, dtype):
    for n_slab in (1, 3):
        for bias in (False, True):
            c = act_case(T, N, n_slab, bias)
            v = R.slab_sum(c["slabs"], c["bias"])
            # act = none: the slab + bias sum itself, bit for bit (rounded to nearest even in bf16)
            out = fa.op_encoder_bias_act(c["slabs"], dtype, bias=c["bias"], act=None)
            assert R.same_bits(out, R.as_stored(v, dtype)), (T, N, n_slab, bias)
            for act in ("gelu_tanh", "gelu_erf"):
                out = fa.op_encoder_bias_act(c["slabs"], dtype, bias=c["bias"], act=act)
                g, lim = R.gelu_bound(v, act, dtype)
                assert out.shape == (T, N) and np.isfinite(R.widen(out)).all()
                room = R.worst(R.widen(out) - g, lim)
                _WORST[act + " " + dtype] = max(_WORST.get(act + " " + dtype, 0.0), room)
                print("\nbias_act T=%d N=%d %s slabs %d bias %d %s: error / bound %.3f" % (T, N, dtype, n_slab, bias, act, room), end="")
                assert room <= 1.0, (T, N, n_slab, bias, act, room)


def test_bias_act_repeats_bit_for_bit(fa):
    c = act_case(5, 1536, 3, True)
    for dtype in DTYPES:
        assert R.same_bits(fa.op_encoder_bias_act(c["slabs"], dtype, bias=c["bias"], act="gelu_erf", repeat=3),
                           fa.op_encoder_bias_act(c["slabs"], dtype, bias=c["bias"], act="gelu_erf"))


# ---- pooling ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h", R.POOL_H)
def test_pool_l2(fa, h):
    for lengths in R.POOL_LENGTHS:
        x = pool_case(tuple(lengths), h)
        out = fa.op_encoder_pool_l2(x, lengths, repeat=3 if h == 264 else 1)
        assert out.shape == (len(lengths), h) and out.dtype == np.float32
        decoder_ref.check_normalized(out, R.pool_means(x, lengths), "pool_l2 h=%d lengths %s" % (h, lengths))
        assert (np.abs(np.linalg.norm(out.astype(np.float64), axis=1) - 1.0) <= 1e-5).all()
        if len(lengths) == 1:
            continue
        # the rows of every other member filled with +-30: the members in between must not move by a bit
        off = np.concatenate([[0], np.cumsum(lengths)])
        for changed in ((1, 3), (0, 2)):
            y = np.array(x, copy=True)
            for s in changed:
                y[off[s]:off[s + 1]] = 30.0 * (1 - 2 * ((np.arange(h) + s) % 2))
            other = fa.op_encoder_pool_l2(y, lengths)
            for s in range(len(lengths)):
                assert R.same_bits(out[s], other[s]) == (s not in changed), (h, changed, s)
