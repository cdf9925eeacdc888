"""Residual add -> RMSNorm -> projection in every fused form, each alone against the exact reference of tests/norm_ref.py:
launch_rmsnorm_add, the row scale in every projection kernel, the norm prologues of the single-sequence, FP8 and batched weight
streams, the residual epilogue of the prefill GEMMs (h += y, xn, partial sums of squares) and the projections that consume its
partial sums.  Rows of a multi-row input differ in magnitude by powers of two (norm_ref.row_scales): a 1/rms taken from another row
is off by a factor of two at least."""
import contextlib
import os

import numpy as np
import pytest

import norm_ref as R
import synth
from conftest import needs_experimental

pytestmark = pytest.mark.gpu
EPS = R.EPS


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


def kernel_name(fa, kernels):
    return fa.LK_NAMES[int(kernels[0])]


# ---- 1. launch_rmsnorm_add -------------------------------------------------------------------------------------------------------
# h: one partial round of 256 x 8 (8, 520), exactly one (2048), one chunk into the second (2056), model widths; n_slab across the
# four-at-a-time loop of the slab sum
@pytest.mark.parametrize("h", [8, 520, 2048, 2056, 3584, 4096])
@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_rmsnorm_add(fa, h, dtype):
    for T in (1, 5):
        for n_slab in (0, 1, 3, 4, 5, 8):
            x, delta, w = R.inputs(T, h, n_slab, 100 + h + n_slab)
            x_new, xs, inv = fa.op_rmsnorm_add(x, delta, w, EPS, dtype)
            v = R.residual(x, delta)
            msg = "T=%d n_slab=%d" % (T, n_slab)
            np.testing.assert_array_equal(x_new, v, err_msg=msg)                 # (a null delta: x_res unchanged)
            np.testing.assert_array_equal(xs, R.xs_of(v, w, dtype), err_msg=msg)
            np.testing.assert_allclose(inv, R.inv_rms(v), rtol=R.INV_RTOL, atol=0, err_msg=msg)


# ---- 2. form 0: the row scale in every projection kernel --------------------------------------------------------------------------
def _form0(fa, T, N, K, dtype, epi, bias, n_slab=2, seed=0):
    """rmsnorm_add + launch_linear(row_scale) on (T, N, K) -- N: rows of W (gate | up for epilogue 1) -- against the reference;
    returns the kernel's name"""
    x, delta, w = R.inputs(T, K, n_slab, 200 + seed + T + N + K)
    W, b = R.weights(N, K, 300 + seed + N, bias)
    Wd, Wv = R.as_dtype(W, dtype)
    y, x_out, kernels = fa.op_norm_linear(0, Wd, w, EPS, x_res=x, delta=delta, bias=b, epilogue=epi)
    v = R.residual(x, delta)
    np.testing.assert_array_equal(x_out, v)
    atol, rtol = R.proj_tol(K, epi)
    np.testing.assert_allclose(y, R.project(R.xs_of(v, w, dtype), R.inv_rms(v), Wv, b, epi), atol=atol, rtol=rtol)
    return kernel_name(fa, kernels)


# (kernel, tune rows, environment, (T, N, K), bias): every shape has a ragged last row tile of its kernel; a bias means one K slab
FORM0_BF16 = [
    ("gemv", {}, {}, (1, 300, 384), True),
    ("dma", {}, {"FL_OP_LINEAR_DMA": 1}, (7, 1000, 256), False),
    ("dma", {}, {"FL_OP_LINEAR_DMA": 1}, (17, 1000, 1024), False),
    ("skinny", {}, {}, (33, 520, 512), True),
    ("skinny", {}, {}, (129, 1000, 1024), False),
    ("skf", {"gemm_skf": 3}, {}, (33, 1000, 1024), False),
    ("h4", {"gemm_h4": 2, "h4_split": 1}, {}, (257, 520, 1024), True),
    ("h4", {"gemm_h4": 2, "h4_split": 3}, {}, (257, 520, 1024), False),
    ("w14", {"gemm_w14": 2, "gemm_h4": 0}, {}, (300, 448, 192), True),
    ("8p", {}, {"FL_GEMM_8P": 2, "FL_GEMM_4W": 0, "FL_GEMM_SKINNY": 0}, (257, 520, 256), True),
    ("8p", {}, {"FL_GEMM_8P": 2, "FL_GEMM_4W": 2, "FL_GEMM_SKINNY": 0}, (257, 520, 256), False),
    ("128", {"gemm_h4": 0}, {"FL_GEMM_8P": 0, "FL_GEMM_SKINNY": 0}, (257, 1000, 1024), True),
    # (two row tiles whose 256 x 128 grid in four K slabs is exactly one round of the chip, as test_linear_plain reaches that kernel)
    ("256", {"gemm_h4": 0}, {"FL_GEMM_8P": 0, "FL_GEMM_SKINNY": 0}, (500, 4096, 4096), False),
    ("generic", {}, {}, (64, 136, 72), True),
]


@pytest.mark.parametrize("kernel,tune,env,shape,bias", FORM0_BF16, ids=lambda v: str(v).replace(" ", "") if not isinstance(v, dict) else "")
def test_form0_row_scale_bf16(fa, kernel, tune, env, shape, bias):
    with switches(fa, env, **tune):
        assert _form0(fa, *shape, "bf16", 0, bias) == kernel


@pytest.mark.parametrize("kernel,tune,shape", [(None, {}, (300, 2 * 704, 512)), ("w14", {"gemm_w14": 2, "gemm_h4": 0}, (300, 2 * 672, 512))])
def test_form0_row_scale_gate_up(fa, kernel, tune, shape):
    """silu(gate) * up behind the row scale: on the default plan, and on the 224-column tile (its width must be whole tiles: 2 x 672)"""
    with switches(fa, **tune):
        ran = _form0(fa, *shape, "bf16", 1, False)
        assert kernel is None or ran == kernel


@pytest.mark.parametrize("kernel,tune,shape,bias", [("gemv", {}, (1, 300, 384), True), ("f32_rows", {}, (17, 520, 1280), True),
                                                    ("f32_mfma", {}, (130, 1000, 1040), True), ("generic", {"force_generic_gemm": 1}, (70, 136, 72), True)])
def test_form0_row_scale_f32(fa, kernel, tune, shape, bias):
    with switches(fa, **tune):
        assert _form0(fa, *shape, "f32", 0, bias) == kernel


# ---- 3. form 1: the norm prologue of the single-sequence stream --------------------------------------------------------------------
# K: below one chunk row, a partial last chunk, the two K with the special U, the prologue's limit.  With so few rows the workgroups
# have four waves: bf16 K = 2048 is the SMALL form's (one chunk of 8 per staging thread: 4 x 64 x 8 = K), every other K the 3-chunk form's
@pytest.mark.parametrize("K", [24, 520, 2048, 2568, 3584, 4096, 6144])
@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_form1_gemv_norm_prologue(fa, K, dtype):
    for N in (2, 33, 300):
        W, b = R.weights(N, K, 400 + N + K, bias=True)
        Wd, Wv = R.as_dtype(W, dtype)
        for n_slab in (1, 2, 8, 9):                                       # across the seven-per-round-trip loop
            x, delta, w = R.inputs(1, K, n_slab, 500 + K + n_slab)
            y, x_out, _ = fa.op_norm_linear(1, Wd, w, EPS, x_res=x, delta=delta, bias=b, repeat=2)
            v = R.residual(x, delta)
            msg = "N=%d n_slab=%d" % (N, n_slab)
            np.testing.assert_array_equal(x_out, v, err_msg=msg)
            atol, rtol = R.proj_tol(K, 0)
            np.testing.assert_allclose(y, R.project(R.xs_of(v, w, dtype), R.inv_rms(v), Wv, b), atol=atol, rtol=rtol, err_msg=msg)
            if n_slab == 1:                                               # the same data through rmsnorm_add + the row-scaled GEMV
                y0, x0, _ = fa.op_norm_linear(0, Wd, w, EPS, x_res=x, delta=delta, bias=b)
                np.testing.assert_array_equal(x0, x_out, err_msg=msg)
                np.testing.assert_allclose(y, y0, atol=atol, rtol=rtol, err_msg=msg)


def test_form1_small_form_at_a_model_width(fa):
    """Mistral-7B's QKV shape: 3072 row groups on 256 twelve-wave workgroups, one group per wave and one chunk per staging thread --
    the SMALL form at K = 4096 (launch_gemv_t's rule; the library has no way to tell which form ran)"""
    N, K = 6144, 4096
    W, b = R.weights(N, K, 450, bias=True)
    Wd, Wv = R.as_dtype(W, "bf16")
    for n_slab in (1, 2):
        x, delta, w = R.inputs(1, K, n_slab, 460 + n_slab)
        y, x_out, _ = fa.op_norm_linear(1, Wd, w, EPS, x_res=x, delta=delta, bias=b, repeat=2)
        v = R.residual(x, delta)
        np.testing.assert_array_equal(x_out, v)
        atol, rtol = R.proj_tol(K, 0)
        np.testing.assert_allclose(y, R.project(R.xs_of(v, w, "bf16"), R.inv_rms(v), Wv, b), atol=atol, rtol=rtol)


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
@pytest.mark.parametrize("epi", [0, 1])
def test_form1_embedding_row_and_gate_up(fa, dtype, epi):
    """layer 0: the normed vector is the embedding row of the step state's token (not token 0); and the gate/up epilogue"""
    K, V, tok = 520, 7, 5
    N = 2 * 88 if epi else 33
    rs = np.random.RandomState(11)
    E = (rs.standard_normal((V, K)) * np.float32(2.0) ** np.arange(V)[:, None]).astype(np.float32)       # every row another magnitude
    Ed, Ev = R.as_dtype(E, dtype)
    W, _ = R.weights(N, K, 12)
    Wd, Wv = R.as_dtype(W, dtype)
    w = R.inputs(1, K, 0, 13)[2]
    y, x_out, _ = fa.op_norm_linear(1, Wd, w, EPS, embed=Ed, tokens=[tok], epilogue=epi)
    v = Ev[tok:tok + 1]
    np.testing.assert_array_equal(x_out, v)
    atol, rtol = R.proj_tol(K, epi)
    np.testing.assert_allclose(y, R.project(R.xs_of(v, w, dtype), R.inv_rms(v), Wv, None, epi), atol=atol, rtol=rtol)


@pytest.mark.parametrize("form,dtype", [(1, "bf16"), (1, "f32"), (2, "bf16")])
def test_norm_prologue_limit_is_unsupported(fa, form, dtype):
    """K = 6152 is past what a workgroup's staging threads hold: FL_ERR_UNSUPPORTED, never another kernel"""
    K = 6160 if form == 2 else 6152
    W = np.zeros((4, K), np.uint8 if form == 2 else (np.uint16 if dtype == "bf16" else np.float32))
    with pytest.raises(fa.FastLLMError) as e:
        fa.op_norm_linear(form, W, np.ones(K), EPS, x_res=np.ones((1, K)), w_scale=np.ones(4) if form == 2 else None)
    assert e.value.code == -10


# ---- 4. form 2: the same prologue over FP8 weights ---------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [16, 528, 4096])
@pytest.mark.parametrize("epi", [0, 1])
def test_form2_w8_norm_prologue(fa, K, epi):
    from test_w8_abi import dequantize
    N = 2 * 88 if epi else 33
    W, b = R.weights(N, K, 600 + K, bias=not epi)
    q, s = fa.op_quantize_rows(W)
    Wv = dequantize(q, s)
    for n_slab in (0, 1):
        x, delta, w = R.inputs(1, K, n_slab, 700 + K + n_slab)
        y, x_out, _ = fa.op_norm_linear(2, q, w, EPS, x_res=x, delta=delta, bias=b, w_scale=s, epilogue=epi, repeat=2)
        v = R.residual(x, delta)
        np.testing.assert_array_equal(x_out, v)
        atol, rtol = R.proj_tol(K, epi)
        np.testing.assert_allclose(y, R.project(R.xs_of(v, w, "bf16"), R.inv_rms(v), Wv, b, epi), atol=atol, rtol=rtol)


# ---- 5. form 3: the batched stream ----------------------------------------------------------------------------------------------
def _form3(fa, B, K, pro, epi, n_slab, seed):
    N = 2 * 176 if epi else 300                                            # 300: a ragged last 32-row unit
    W, b = R.weights(N, K, 800 + K + epi, bias=not epi and K <= 4096)
    Wd, Wv = R.as_dtype(W, "bf16")
    atol, rtol = R.proj_tol(K, epi)
    msg = "B=%d K=%d pro=%d epi=%d n_slab=%d" % (B, K, pro, epi, n_slab)
    if pro == 0:
        # no norm here, so no row scale either: x as tests/test_gpu_ops.py draws it
        xd, xv = R.as_dtype(np.random.RandomState(seed).standard_normal((B, K)).astype(np.float32), "bf16")
        y, _, kernels = fa.op_norm_linear(3, Wd, x=xd, pro=0, bias=b, epilogue=epi, repeat=4)
        np.testing.assert_allclose(y, R.project(xv, np.ones(B), Wv, b, epi), atol=atol, rtol=rtol, err_msg=msg)
        return kernels
    x, delta, w = R.inputs(B, K, n_slab, seed)
    y, x_out, kernels = fa.op_norm_linear(3, Wd, w, EPS, x_res=x, delta=delta, bias=b, epilogue=epi, repeat=4)
    v = R.residual(x, delta)
    np.testing.assert_array_equal(x_out, v, err_msg=msg)
    np.testing.assert_allclose(y, R.project(R.xs_of(v, w, "bf16"), R.inv_rms(v), Wv, b, epi), atol=atol, rtol=rtol, err_msg=msg)
    return kernels


# VALU kernels NB = 2 / 4 / 8 with B < NB padding (batch_mfma_min = 9 keeps the MFMA forms out), and the MFMA forms by batch_mode;
# K = 520: K % 32 != 0, the VALU kernels whatever the mode
@pytest.mark.parametrize("mode,Bs", [("valu", (1, 2, 3, 5, 8)), (0, (3, 8)), (1, (3, 8)), (2, (3, 8))])
@pytest.mark.parametrize("K", [520, 1024, 4096])
def test_form3_batched_stream(fa, mode, Bs, K):
    tune = {"batch_mfma_min": 9} if mode == "valu" else {"batch_mode": mode}
    with switches(fa, **tune):
        for B in Bs:
            for pro in (0, 1):
                for epi in (0, 1):
                    for n_slab in ((1, 3) if pro else (0,)):
                        _form3(fa, B, K, pro, epi, n_slab, 900 + B + K)


@pytest.mark.parametrize("mode", ["valu", 2])
def test_form3_k_slices(fa, mode):
    """K = 14336: eight rows of it do not fit LDS, the launch runs in K slices whose slabs are summed in slab order"""
    with switches(fa, **({"batch_mfma_min": 9} if mode == "valu" else {"batch_mode": mode})):
        for B in (3, 8):
            kernels = _form3(fa, B, 14336, 0, 0, 0, 950 + B)
            assert kernels[1] > 1, kernels


def test_form3_embedding_rows(fa):
    """every sequence's own token from its own step state"""
    K, V, B, N = 1024, 9, 5, 300
    rs = np.random.RandomState(21)
    Ed, Ev = R.as_dtype((rs.standard_normal((V, K)) * np.float32(2.0) ** (np.arange(V) - 4)[:, None]).astype(np.float32), "bf16")
    Wd, Wv = R.as_dtype(R.weights(N, K, 22)[0], "bf16")
    w = R.inputs(1, K, 0, 23)[2]
    toks = [7, 2, 8, 2, 4]
    for tune in ({"batch_mfma_min": 9}, {}):
        with switches(fa, **tune):
            y, x_out, _ = fa.op_norm_linear(3, Wd, w, EPS, embed=Ed, tokens=toks, repeat=2)
        v = Ev[toks]
        np.testing.assert_array_equal(x_out, v)
        atol, rtol = R.proj_tol(K, 0)
        np.testing.assert_allclose(y, R.project(R.xs_of(v, w, "bf16"), R.inv_rms(v), Wv), atol=atol, rtol=rtol)


# ---- 6. the residual epilogue, integer operands --------------------------------------------------------------------------------------
def _int_case(T, N, K, bias, seed):
    """x, W in -3..3 and h_in in -8..8, rows of x and h_in times the row scale (a power of two); an integer bias; w_next uniform in
    [0.5, 1.5].  Every product and partial sum is an integer multiple of the row's power of two below 2^24 of them, so h + y (+ bias)
    is exact in fp32 in ANY summation order, and a float32 BLAS product is the exact reference."""
    rs = np.random.RandomState(seed)
    sc = R.row_scales(T)
    x = rs.randint(-3, 4, size=(T, K)).astype(np.float32) * sc
    W = rs.randint(-3, 4, size=(N, K)).astype(np.float32)
    h_in = rs.randint(-8, 9, size=(T, N)).astype(np.float32) * sc
    b = rs.randint(-8, 9, size=N).astype(np.float32) if bias else None
    w_next = rs.uniform(0.5, 1.5, size=N).astype(np.float32)
    assert 9 * K * 32 + 16 * 32 < 2 ** 24
    y = x @ W.T
    h = h_in + (y + b if bias else y)
    return synth.f32_to_bf16_bits(x), synth.f32_to_bf16_bits(W), h_in, b, w_next, h


def _check_resid(out, h, w_next, N, msg=""):
    """h bit for bit; xn = bf16(float32(h * w_next)) bit for bit; every partial-sum slot written, the slots behind the last 64-column
    strip exactly zero; 1/rms (when the call finalized it) within the partial-sum tolerance"""
    np.testing.assert_array_equal(out["h"], h, err_msg=msg)
    np.testing.assert_array_equal(out["xn"], R.xs_of(h, w_next, "bf16"), err_msg=msg)
    part = out["part"]
    np_ = part.shape[1]
    assert np_ == (N + 255) // 256 * 4 and not np.isnan(part).any(), msg
    strips = (N + 63) // 64
    assert (part[:, strips:] == 0).all(), msg
    ss = (h.astype(np.float64) ** 2).sum(axis=1)
    np.testing.assert_allclose(part.astype(np.float64).sum(axis=1), ss, rtol=R.inv_parts_rtol(np_), atol=0, err_msg=msg)
    if not np.isnan(out["inv_rms"]).any():
        np.testing.assert_allclose(out["inv_rms"], R.inv_rms(h), rtol=R.inv_parts_rtol(np_), atol=0, err_msg=msg)


# N: 256 k + 16, not a multiple of 64, a model width (Qwen2-0.5B's 896, 4096); wait_us = 0: every early slice abandons its blocks at
# once and the slice counted last finishes them from memory (the rescue path)
@pytest.mark.parametrize("T,N,K", [(130, 272, 256), (257, 896, 512), (300, 1104, 1024), (512, 4096, 4096)])
@pytest.mark.parametrize("slices,wait_us", [(1, 30), (2, 30), (3, 30), (4, 30), (2, 0), (3, 0), (4, 0)])      # (one slice has nobody to wait for)
def test_resid_h4(fa, T, N, K, slices, wait_us):
    xb, wb, h_in, b, w_next, h = _int_case(T, N, K, bias=(slices % 2 == 0), seed=T + N + K + slices)
    with switches(fa, gemm_h4=2, h4_split=slices, h4_wait_us=wait_us):
        for lazy in (False, True):
            out = fa.op_linear_resid(xb, wb, h_in, w_next, EPS, bias=b, lazy=lazy, repeat=6 if not lazy else 1)
            assert out["kernels"]["kernel"] == "h4" and out["kernels"]["ks"] == slices, out["kernels"]
            assert not np.isnan(out["inv_rms"]).any()
            _check_resid(out, h, w_next, N, "lazy=%s" % lazy)


# 256 x 256 whole: the planner takes the residual epilogue there from about 2048 rows of a model-wide matrix (gemm_resid_8p_wins;
# smaller shapes lose to K slabs + rmsnorm_add and are declined): a ragged row tile with N = 256 k + 16, and a model width
@pytest.mark.parametrize("T,N,K", [(2100, 4112, 512), (3000, 3584, 512), (2100, 4096, 1024)])
def test_resid_8p_whole(fa, T, N, K):
    xb, wb, h_in, b, w_next, h = _int_case(T, N, K, bias=(N == 4112), seed=T + N + K)
    with switches(fa, gemm_h4=0):
        out = fa.op_linear_resid(xb, wb, h_in, w_next, EPS, bias=b, repeat=2)
    assert out["kernels"]["kernel"] == "8p" and out["kernels"]["tail"] == "none", out["kernels"]
    _check_resid(out, h, w_next, N)


@pytest.mark.parametrize("T,N,K", [(256, 512, 128), (300, 896, 1024), (513, 4096, 4096)])
def test_resid_declined_shapes_are_unsupported(fa, T, N, K):
    """without the 128 x 256 kernel nothing takes the residual epilogue at these sizes: FL_ERR_UNSUPPORTED, never another kernel"""
    xb, wb, h_in, b, w_next, h = _int_case(T, N, K, bias=False, seed=1)
    with switches(fa, gemm_h4=0):
        with pytest.raises(fa.FastLLMError) as e:
            fa.op_linear_resid(xb, wb, h_in, w_next, EPS)
    assert e.value.code == -10


# whole rounds of 256 x 256 tiles + the tail columns: on the stream-K launch + fix-up (the shapes of test_linear_peeled_columns; the
# 128 x 256 kernel takes a tail from 160 workgroups on: 912 columns at 4096 rows in two slices)
@pytest.mark.parametrize("T,N,K,tail,h4", [(4096, 4352, 1024, "8p_streamk", 1), (4096, 4352, 1024, "8p_streamk", 0), (2048, 8448, 1024, "8p_streamk", 0),
                                          (4096, 5008, 1024, "h4", 1)])
def test_resid_8p_with_tail(fa, T, N, K, tail, h4):
    xb, wb, h_in, b, w_next, h = _int_case(T, N, K, bias=(T == 2048), seed=T + N + K)
    with switches(fa, gemm_h4=h4):
        out = fa.op_linear_resid(xb, wb, h_in, w_next, EPS, bias=b, repeat=2)
    assert out["kernels"]["kernel"] == "8p" and out["kernels"]["tail"] == tail, out["kernels"]
    _check_resid(out, h, w_next, N)


@needs_experimental
@pytest.mark.parametrize("T,N,K", [(2, 320, 256), (33, 896, 1024), (128, 4096, 4096)])
@pytest.mark.parametrize("slices", [1, 2, 3, 4])
def test_resid_skf(fa, T, N, K, slices):
    """the short-prompt GEMM's residual epilogue (whole 64-column strips: N = 272 is declined)"""
    xb, wb, h_in, b, w_next, h = _int_case(T, N, K, bias=(slices % 2 == 0), seed=T + N + K + slices)
    with switches(fa, gemm_skf=3, skf_split=slices):
        out = fa.op_linear_resid(xb, wb, h_in, w_next, EPS, bias=b, repeat=6)
        assert out["kernels"]["kernel"] == "skf" and out["kernels"]["ks"] == slices, out["kernels"]
        _check_resid(out, h, w_next, N)
        if T == 2:
            with pytest.raises(fa.FastLLMError) as e:
                fa.op_linear_resid(*_int_case(2, 272, 256, False, 1)[:2], np.zeros((2, 272), np.float32), np.ones(272), EPS)
            assert e.value.code == -10


def _random_resid(fa, T, N, K, seed):
    """random operands at the projection tolerance, xn within one bf16 ulp: a check that the integer trick hides nothing"""
    rs = np.random.RandomState(seed)
    xd, xv = R.as_dtype(rs.standard_normal((T, K)).astype(np.float32), "bf16")
    Wd, Wv = R.as_dtype(R.weights(N, K, seed + 1)[0], "bf16")
    h_in = rs.standard_normal((T, N)).astype(np.float32)
    w_next = rs.uniform(0.5, 1.5, size=N).astype(np.float32)
    out = fa.op_linear_resid(xd, Wd, h_in, w_next, EPS)
    h = h_in.astype(np.float64) + xv.astype(np.float64) @ Wv.astype(np.float64).T
    atol, rtol = R.proj_tol(K, 0)
    np.testing.assert_allclose(out["h"], h, atol=atol, rtol=rtol)
    np.testing.assert_allclose(out["xn"], out["h"].astype(np.float64) * w_next, atol=0, rtol=2.0 ** -8)
    np_ = out["part"].shape[1]
    np.testing.assert_allclose(out["inv_rms"], R.inv_rms(out["h"]), rtol=R.inv_parts_rtol(np_), atol=0)
    return out["kernels"]


def test_resid_random_data_h4(fa):
    with switches(fa, gemm_h4=2, h4_split=3):
        assert _random_resid(fa, 257, 896, 512, 31)["kernel"] == "h4"


def test_resid_random_data_8p_and_tail(fa):
    with switches(fa, gemm_h4=0):
        assert _random_resid(fa, 2100, 4112, 512, 32)["kernel"] == "8p"
        k = _random_resid(fa, 2048, 8448, 1024, 33)
        assert k["kernel"] == "8p" and k["tail"] == "8p_streamk", k


@needs_experimental
def test_resid_random_data_skf(fa):
    with switches(fa, gemm_skf=3):
        assert _random_resid(fa, 33, 896, 1024, 34)["kernel"] == "skf"


# ---- 7. the consumer of the partial sums --------------------------------------------------------------------------------------------
def _consumer(fa, T, N, K, N2, epi2, lazy, seed, bias=False, cols=None):
    """an integer residual epilogue (xn known bit for bit) and the projection behind it: y2 against fp64 at the projection tolerance
    (cols: only these columns of a plain y2 -- a row scale is wrong in every column of its row)"""
    xb, wb, h_in, b, w_next, h = _int_case(T, N, K, bias, seed)
    W2d, W2v = R.as_dtype(R.weights(N2, N, seed + 5)[0], "bf16")
    out = fa.op_linear_resid(xb, wb, h_in, w_next, EPS, bias=b, w2=W2d, epi2=epi2, lazy=lazy, repeat=2)
    _check_resid(out, h, w_next, N)
    atol, rtol = R.proj_tol(N, epi2)
    y2 = out["y2"]
    assert not np.isnan(y2).any()
    if cols is not None:
        y2, W2v = y2[:, cols], W2v[cols]
    np.testing.assert_allclose(y2, R.project(R.xs_of(h, w_next, "bf16"), R.inv_rms(h), W2v, None, epi2), atol=atol, rtol=rtol)
    return out


# W2 as gate/up (2 x 352 rows) and plain (520 rows: a ragged last tile)
@pytest.mark.parametrize("N2,epi2", [(2 * 352, 1), (520, 0)])
@pytest.mark.parametrize("lazy", [False, True])
def test_consumer_on_h4(fa, N2, epi2, lazy):
    """the 128 x 256 kernel reads the partial sums itself (reads_rs_parts): with lazy nobody ever writes the 1/rms vector"""
    with switches(fa, gemm_h4=2, h4_split=2):
        for T, N, K in ((257, 896, 512), (512, 4096, 4096)):
            out = _consumer(fa, T, N, K, N2, epi2, lazy, T + N2)
            k = out["kernels"]
            assert k["kernel"] == "h4" and k["consumer"] == "h4" and k["consumer_reads_parts"], k
            assert np.isnan(out["inv_rms"]).all() == lazy


@pytest.mark.parametrize("N2,epi2", [(2 * 352, 1), (520, 0)])
@pytest.mark.parametrize("debug", [0, 1])
def test_consumer_through_the_safety_net(fa, N2, epi2, debug):
    """a consumer that takes its row scales as a vector (K = 272 / 1104 are no whole K tiles: the generic kernel) behind a lazy
    epilogue: launch_one finishes the partial sums first (rs_parts_to_vector); debug_rs_parts = 1 plans every shape as reading them"""
    with switches(fa, gemm_h4=2, h4_split=2, debug_rs_parts=debug):
        for T, N, K in ((130, 272, 256), (300, 1104, 1024)):
            out = _consumer(fa, T, N, K, N2, epi2, True, T + N2, bias=True)
            k = out["kernels"]
            assert k["kernel"] == "h4" and k["consumer"] == "generic" and k["consumer_reads_parts"] == bool(debug), k
            np.testing.assert_allclose(out["inv_rms"], R.inv_rms(out["h"]), rtol=R.inv_parts_rtol(out["part"].shape[1]), atol=0)


@pytest.mark.parametrize("lazy", [False, True])
def test_consumer_on_8p(fa, lazy):
    with switches(fa, gemm_h4=0):
        out = _consumer(fa, 3000, 3584, 512, 2 * 352, 1, lazy, 41)
    k = out["kernels"]
    assert k["kernel"] == "8p", k
    nan = np.isnan(out["inv_rms"])                                        # lazy: read in the kernel, or finished by the safety net -- by the plan
    assert nan.all() if lazy and k["consumer_reads_parts"] else not nan.any(), k


@pytest.mark.parametrize("four", [0, 1])                                 # the eight-wave kernel / its four-wave form (from 768 rows)
def test_consumer_on_8p_reads_the_partial_sums(fa, four):
    """a consumer the cost model itself puts on the 256 x 256 kernel whole (2100 x 4096 x 4096: nine row tiles, the last one ragged):
    both forms take 1/rms from the partial sums while they stage the tile's row scales"""
    cols = np.r_[0:130, 4096 - 130:4096]
    with switches(fa, {"FL_GEMM_4W": four}, gemm_h4=0):
        out = _consumer(fa, 2100, 4096, 1024, 4096, 0, True, 61, cols=cols)
    k = out["kernels"]
    assert k["kernel"] == "8p" and k["consumer"] == "8p" and k["consumer_reads_parts"], k
    assert np.isnan(out["inv_rms"]).all()                                  # nobody ever wrote the vector


def test_consumer_gate_up_row_split_behind_a_lazy_epilogue(fa):
    """545 rows of gate/up on the 224-column kernel: 512 on it (partial sums read in the kernel) and the last 33 as a launch of their own
    that starts at partial-sum row 512 (launch_plan's rsp.part += r * np) -- behind the 128 x 256 kernel's residual epilogue, which
    takes 545 rows from N = K = 3072 on by its own rule (with it forced on it would take the consumer too)"""
    T, I, N = 545, 4480, 3072
    with switches(fa, gemm_w14=2):
        out = _consumer(fa, T, N, N, 2 * I, 1, True, 51)
    k = out["kernels"]
    assert k["kernel"] == "h4" and k["consumer"] == "w14", k
    inv = out["inv_rms"]
    assert np.isnan(inv[:512]).all()                                       # the even part never needed the vector
    np.testing.assert_allclose(inv[512:], R.inv_rms(out["h"])[512:], rtol=R.inv_parts_rtol(out["part"].shape[1]), atol=0)
