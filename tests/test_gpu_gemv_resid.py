"""Decode: residual add + RMSNorm finished once in the producer's epilogue (k_gemv.hip EPI_RESID: o_proj / down_proj) and staged ready
by the consumer (PRO_XS: gate/up, the next QKV projection, lm_head) -- each alone against an exact reference, the pair bit for bit
against today's two launches (plain epilogue, then the PRO_NORM prologue) on the same inputs, the shapes the rule declines, and a whole
small model with the switch on and off.  tests/test_gemv_resid_plan.py checks the rule itself without a GPU."""
import numpy as np
import pytest

import norm_ref as R
import rope_ref
import synth

pytestmark = pytest.mark.gpu
EPS = R.EPS
UNSUPPORTED = -10

bits, widen = synth.f32_to_bf16_bits, synth.bf16_bits_to_f32


@pytest.fixture(scope="module")
def fa():
    import fastllm_amd
    assert fastllm_amd.device_count() >= 1
    return fastllm_amd


def u32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---- 1. the producer alone ---------------------------------------------------------------------------------------------------------
# (8, 64): one workgroup, one chunk, a partial K block; (2048, 2048): 256 four-wave workgroups; (4096, 4096): the 8-wave geometry, two
# chunks per workgroup, SMALL; (4096, 14336): PIPE, ragged last block
@pytest.mark.parametrize("N,K", [(8, 64), (16, 1024), (2048, 2048), (4096, 4096), (4096, 14336)])
def test_producer_alone_is_exact(fa, N, K):
    """x, W in {-1, 0, 1}, h_in an integer in [-8, 8]: every partial sum of the dot product, v = h_in + W . x and the chunk sums of
    squares are integers below 2^24 (asserted), so fp32 gives them exactly in any order; v * w_next is one fp32 rounding and one
    RNE rounding to bf16 in the kernel and in numpy alike"""
    rs = np.random.RandomState(1000 + N + K)
    x = rs.randint(-1, 2, size=K).astype(np.float32)
    W = rs.randint(-1, 2, size=(N, K)).astype(np.int8)
    h_in = rs.randint(-8, 9, size=N).astype(np.float32)
    w_next = rs.uniform(0.5, 1.5, size=N).astype(np.float32)
    v = h_in.astype(np.int64) + W.astype(np.int32) @ x.astype(np.int32)
    cs = (v * v).reshape(-1, 8).sum(axis=1)
    assert np.abs(W).sum(axis=1).max() + 8 < 2 ** 24 and cs.max() < 2 ** 24
    out = fa.op_gemv_resid(0, EPS, x=bits(x), w=bits(W.astype(np.float32)), h_in=h_in, w_next=w_next, repeat=2)
    v32 = v.astype(np.float32)
    np.testing.assert_array_equal(out["h"], v32)
    np.testing.assert_array_equal(out["xs"], bits((v32 * w_next).astype(np.float32)))
    np.testing.assert_array_equal(out["cs"], cs.astype(np.float32))
    assert (u32(out["delta"]) == 0xFFFFFFFF).all(), "the producer wrote its `out` buffer"


# ---- 2. the consumer alone ---------------------------------------------------------------------------------------------------------
def consumer_case(K, epi2):
    """(w2 rows, rope shape): at K = 4096 the matrix must fill the chip with 8 waves per workgroup or more (512 chunks to stage)"""
    big = K >= 4096
    if epi2 == 0:
        return (4100 if big else 300), None
    if epi2 == 1:
        return 2 * (2064 if big else 352), None
    H, Hkv, d = (16, 8, 128) if big else (4, 2, 64)
    return (H + 2 * Hkv) * d, (H, Hkv, d)


def rope_args(shape, pos=5, length=7, seq_alloc=32, max_pos=16):
    H, Hkv, d = shape
    cos, sin = rope_ref.tables(max_pos, d)
    return dict(H=H, Hkv=Hkv, d=d, pos=pos, len=length, seq_alloc=seq_alloc, cos=cos, sin=sin)


def check_consumer(y, v, w, W2v, epi2, shape, K, rope=None):
    """y of a consumer launch against norm_ref.project on the exact xs and 1/rms, at norm_ref.proj_tol (QKV: that bound through the
    rotation and the rounding to the cache dtype, rope_ref.fused_bounds)"""
    xs, inv = R.xs_of(v, w, "bf16"), R.inv_rms(v)
    if epi2 < 2:
        atol, rtol = R.proj_tol(K, epi2)
        np.testing.assert_allclose(y[None, :], R.project(xs, inv, W2v, None, epi2), atol=atol, rtol=rtol)
        return
    H, Hkv, d = shape
    pos = np.array([rope["pos"]])
    want, lims = rope_ref.fused_bounds(R.project(xs, inv, W2v), rope["cos"], rope["sin"], pos, H, Hkv, d, K, "bf16")
    got = (y[:H * d], y[H * d:(H + Hkv) * d], y[(H + Hkv) * d:])
    for name, g, r, lim in zip("qkv", got, want, lims):
        err = np.abs(g.astype(np.float64) - r[0])
        assert (err <= lim[0]).all(), (name, (err / np.maximum(lim[0], 1e-30)).max())


@pytest.mark.parametrize("epi2", [0, 1, 2], ids=["f32_amax", "gateup", "qkv_rope"])
@pytest.mark.parametrize("K", [64, 4096])
def test_consumer_alone(fa, K, epi2):
    N2, shape = consumer_case(K, epi2)
    x, delta, w = R.inputs(1, K, 1, 2000 + K + epi2)
    v = R.residual(x, delta)
    W2 = R.weights(N2, K, 2100 + N2)[0]
    W2d, W2v = R.as_dtype(W2, "bf16")
    xs_bits = bits((v[0] * w).astype(np.float32))
    cs = (v[0].astype(np.float64) ** 2).reshape(-1, 8).sum(axis=1).astype(np.float32)
    rope = rope_args(shape) if shape else None
    out = fa.op_gemv_resid(1, EPS, xs=xs_bits, cs=cs, w2=W2d, epi2=epi2, rope=rope, repeat=2)
    check_consumer(out["y"], v, w, W2v, epi2, shape, K, rope)
    np.testing.assert_allclose(out["inv"][0], R.inv_rms(v)[0], rtol=R.INV_RTOL, atol=0)
    if epi2 == 0:                                            # the workgroups' ArgMax candidates: ties to the larger index
        y = out["y"]
        assert out["amax"] == int(np.flatnonzero(y == y.max())[-1])


# ---- 3. the pair, bit for bit against today's two launches --------------------------------------------------------------------------
def pair_case(h, epi2):
    """(producer K, w2 rows, rope shape) at width h.  h = 4096 takes consumers of 8 waves or more; 256 is the synthetic model's width"""
    if h == 4096:
        N2, shape = consumer_case(4096, epi2)
        return 1024, N2, shape
    Kp = 352 if h == 256 else 2048
    if epi2 == 0:
        return Kp, 1000, None
    if epi2 == 1:
        return Kp, 2 * 352, None
    return Kp, 512, (4, 2, 64)


@pytest.mark.parametrize("epi2", [0, 1, 2], ids=["f32_amax", "gateup", "qkv_rope"])
@pytest.mark.parametrize("h", [256, 2048, 4096])
def test_pair_is_bitwise_todays_two_launches(fa, h, epi2):
    """random bf16-range data; y, h and 1/m of (EPI_RESID, PRO_XS) equal those of (EPI_F32, PRO_NORM) bit for bit, run twice (the op
    refuses a second run that gives other bytes); and both are right"""
    Kp, N2, shape = pair_case(h, epi2)
    rs = np.random.RandomState(3000 + h + epi2)
    x = rs.standard_normal(Kp).astype(np.float32)
    W = R.weights(h, Kp, 3100 + h)[0]
    Wd, Wv = R.as_dtype(W, "bf16")
    h_in, _, w_next = R.inputs(1, h, 0, 3200 + h)
    W2 = R.weights(N2, h, 3300 + N2 + h)[0]
    W2d, W2v = R.as_dtype(W2, "bf16")
    rope = rope_args(shape) if shape else None
    out = fa.op_gemv_resid(2, EPS, x=bits(x), w=Wd, h_in=h_in[0], w_next=w_next, w2=W2d, epi2=epi2, rope=rope, repeat=2)
    for key in ("h", "y", "inv"):
        np.testing.assert_array_equal(u32(out[key]), u32(out[key + "_ref"]), err_msg=key)
    assert out["amax"] == out["amax_ref"]
    assert (u32(out["delta"]) == 0xFFFFFFFF).all()
    # ... and xs, cs are what the norm prologue computes from that h: one product and one RNE; the fmaf chain from 0 in element order
    hv = out["h"]
    np.testing.assert_array_equal(out["xs"], bits((hv * w_next).astype(np.float32)))
    chain = np.zeros(h // 8, np.float64)
    for j in range(8):                                       # fmaf(v, v, ss): the exact v^2 + ss rounded once (float64 holds it exactly)
        e = hv.reshape(-1, 8)[:, j].astype(np.float64)
        chain = (e * e + chain).astype(np.float32).astype(np.float64)
    np.testing.assert_array_equal(out["cs"], chain.astype(np.float32))
    # the values themselves: h against the float64 projection, y through the reference of the consumer
    xb = widen(bits(x)).astype(np.float64)
    want_h = h_in[0].astype(np.float64) + Wv.astype(np.float64) @ xb
    atol, rtol = R.proj_tol(Kp, 0)
    np.testing.assert_allclose(hv, want_h, atol=atol + 1e-6, rtol=rtol)
    check_consumer(out["y"], hv[None, :], w_next, W2v, epi2, shape, h, rope)
    np.testing.assert_allclose(out["inv"][0], R.inv_rms(hv[None, :])[0], rtol=R.INV_RTOL, atol=0)


# ---- 4. what the rule declines -------------------------------------------------------------------------------------------------------
def _producer(fa, N, K, seed=5):
    rs = np.random.RandomState(seed)
    return fa.op_gemv_resid(0, EPS, x=bits(rs.standard_normal(K).astype(np.float32)), w=bits(rs.standard_normal((N, K)).astype(np.float32) * 0.05),
                            h_in=rs.standard_normal(N).astype(np.float32), w_next=np.ones(N, np.float32))


def test_declined_shapes_report_unsupported(fa):
    """N = 3584 (256 x 7 waves: 14 rows per workgroup), a forced grid, and a consumer with fewer staging threads than chunks"""
    with pytest.raises(fa.FastLLMError) as e:
        _producer(fa, 3584, 512)
    assert e.value.code == UNSUPPORTED
    try:
        fa.tune("gemv_blocks", 64); fa.tune("gemv_waves", 8)
        with pytest.raises(fa.FastLLMError) as e:
            _producer(fa, 4096, 512)                          # (64 x 8 x 2 rows do not cover it either; the forced grid is refused first)
        assert e.value.code == UNSUPPORTED
    finally:
        fa.tune("gemv_blocks", 0); fa.tune("gemv_waves", 0)
    _producer(fa, 4096, 512)
    x, delta, w = R.inputs(1, 4096, 1, 77)
    v = R.residual(x, delta)[0]
    cs = (v.astype(np.float64) ** 2).reshape(-1, 8).sum(axis=1).astype(np.float32)
    with pytest.raises(fa.FastLLMError) as e:                 # 512 rows: 64 workgroups of 4 waves, 256 threads for 512 chunks
        fa.op_gemv_resid(1, EPS, xs=bits(v), cs=cs, w2=bits(R.weights(512, 4096, 78)[0]), epi2=0)
    assert e.value.code == UNSUPPORTED


# ---- 5. a whole model ------------------------------------------------------------------------------------------------------------------
NP, NGEN = 40, 16


def _run_model(fa, cache_len, **tune):
    """llama_a (bf16, h = 256, 2 layers): a 40-token prompt, 16 greedy tokens, then one more forward for the logits row; returns
    (tokens, logits, the kernel names of one decode step)"""
    cfg = synth.CONFIGS["llama_a"]
    ids = synth.prompt_ids(cfg, NP, seed=11)
    try:
        for k, val in tune.items():
            fa.tune(k, val)
        gm = fa.Model(cfg, synth.synth_weights(cfg), dtype="bf16")
        c = gm.new_cache(cache_len)
        first = gm.forward_argmax(c, ids, 0)
        toks = gm.decode_greedy(c, first, NP, NGEN)
        gm.profile_begin()
        logits = gm.forward(c, toks[-1:], NP + NGEN)
        names = sorted(s["name"] for s in gm.profile_end())
        c.close()
        gm.close()
    finally:
        fa.tune("reload_env", 0)
        fa.tune("gemv_blocks", 0); fa.tune("gemv_waves", 0)
    return np.concatenate([[first], toks]), logits, names


@pytest.fixture(scope="module")
def model_off(fa):
    """the reference runs, computed once: the switch off, for a cache past the replicated-attention limit and a short one"""
    return {n: _run_model(fa, n, gemv_resid=0) for n in (512, 64)}


def tagged(names, tag):
    return [n for n in names if n.startswith("gemv[") and ("," + tag) in n]


@pytest.mark.parametrize("cache_len", [512, 64])
def test_whole_model_equal_with_the_switch_on_and_off(fa, model_off, cache_len):
    """gemv_resid 1 (the default) and 2 (the same launches, their tags naming the form) against 0.  By default a launch keeps the name
    it has always had -- the recorded kernel lists of tests/test_gpu_kernel_selection.py know the decode step by those names"""
    toks0, lg0, names0 = model_off[cache_len]
    toks_d, lg_d, names_d = _run_model(fa, cache_len, gemv_resid=1)
    np.testing.assert_array_equal(toks_d, toks0)
    np.testing.assert_array_equal(u32(lg_d), u32(lg0))
    assert names_d == names0, (names_d, names0)
    toks1, lg1, names1 = _run_model(fa, cache_len, gemv_resid=2)
    np.testing.assert_array_equal(toks1, toks0)
    np.testing.assert_array_equal(u32(lg1), u32(lg0))
    assert not tagged(names0, "resid") and not tagged(names0, "xs"), names0
    rep = any(n.startswith("attn_oproj[rep") for n in names1)
    assert rep == (cache_len == 64), names1
    if rep:    # the o_proj edge keeps the norm prologue (the replicated launch is no producer); down_proj -> next QKV / lm_head take the new form
        assert tagged(names1, "resid") == ["gemv[256x352,resid]"], names1
        assert tagged(names1, "xs") == ["gemv[256x256,xs]", "gemv[512x256,xs,rope]"], names1
        assert "gemv[704x256,norm,glu]" in names1, names1
    else:
        assert tagged(names1, "resid") == ["gemv[256x256,resid]", "gemv[256x352,resid]"], names1
        assert tagged(names1, "xs") == ["gemv[256x256,xs]", "gemv[512x256,xs,rope]", "gemv[704x256,xs,glu]"], names1
        assert tagged(names1, "norm") == ["gemv[512x256,norm,rope]"], names1          # layer 0: the embedding row


def test_a_forced_grid_falls_back_to_the_norm_prologue(fa):
    """the step builder asks the rule per edge: under fl_tune gemv_blocks / gemv_waves every edge keeps PRO_NORM, and the tokens are
    those of the same grid with the switch off"""
    toks0, lg0, _ = _run_model(fa, 512, gemv_resid=0, gemv_blocks=16, gemv_waves=4)
    toks1, lg1, names = _run_model(fa, 512, gemv_resid=2, gemv_blocks=16, gemv_waves=4)
    assert not tagged(names, "resid") and not tagged(names, "xs"), names
    assert len(tagged(names, "norm")) == 3, names
    np.testing.assert_array_equal(toks1, toks0)
    np.testing.assert_array_equal(u32(lg1), u32(lg0))
