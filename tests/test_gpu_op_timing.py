"""The timed path of the op entry points (fl_op_linear, fl_op_gemv_w8, fl_op_kv_copy with iters > 0): one launch, a warming launch
on every rotating copy of the working set, then `iters` launches between two events.

The time itself has no bound here (finite and positive is all).  What is checked is that the rotation leaves the result alone: the
output of a timed call equals the output of the same call with iters = 0 bit for bit, under op_hot = 0 (the default rule: 24 copies
at these sizes), 1 (one copy) and 2 (iters = 3: the rotation wraps).  These kernels sum in a fixed order -- the split-K slabs are
added on the host in slab order, the copy is idempotent -- so every launch on every copy writes the same bits (it held for every case below before the three ops came to share one timing
loop, too)."""
import numpy as np
import pytest

import synth

pytestmark = pytest.mark.gpu

HOT = [0, 1, 2]


@pytest.fixture(scope="module")
def fa():
    import fastllm_amd
    assert fastllm_amd.device_count() >= 1, "no MI355X visible"
    return fastllm_amd


def _bits(shape, seed, scale=1.0):
    return synth.f32_to_bf16_bits((np.random.RandomState(seed).standard_normal(shape) * scale).astype(np.float32))


_untimed = {}


def check(fa, hot, iters, key, call):
    """call(iters) under op_hot = hot against call(0) (computed once per case)"""
    if key not in _untimed:
        _untimed[key] = call(0)
    want = _untimed[key]
    fa.tune("op_hot", hot)
    try:
        got, ms = call(iters)
    finally:
        fa.tune("op_hot", 0)                  # the tune table is process-wide
    print("%s op_hot %d: %.6f ms per launch" % (key, hot, ms))
    assert np.isfinite(ms) and ms > 0, ms
    assert got.dtype == want.dtype and got.shape == want.shape
    assert not np.isnan(want).any()
    assert got.tobytes() == want.tobytes(), np.argwhere(got != want)[:8]


# (T, N, K, epilogue, iters): the decode GEMV plain (no bias: the op allows split-K slabs) and gate/up with I = 24 (the 16-row padding
# of gate/up is live), and one prompt-shaped launch
LINEAR = [(1, 96, 64, 0, 3), (1, 48, 64, 1, 3), (33, 128, 128, 0, 2)]


@pytest.mark.parametrize("hot", HOT)
@pytest.mark.parametrize("T,N,K,epi,iters", LINEAR)
def test_linear_timed_equals_untimed(fa, T, N, K, epi, iters, hot):
    x, w = _bits((T, K), 1), _bits((N, K), 2, 0.05)
    check(fa, hot, iters, ("linear", T, N, K, epi), lambda it: fa.op_linear(x, w, None, epilogue=epi, iters=it))


@pytest.mark.parametrize("hot", HOT)
@pytest.mark.parametrize("epi", [0, 1])
def test_gemv_w8_timed_equals_untimed(fa, epi, hot):
    N, K = 48, 64
    q, s = fa.op_quantize_rows(_bits((N, K), 3, 0.05))
    x = _bits((K,), 4)
    bias = None if epi else np.random.RandomState(5).standard_normal(N).astype(np.float32)
    check(fa, hot, 3, ("gemv_w8", epi), lambda it: fa.op_gemv_w8(x, q, s, bias=bias, epilogue=epi, iters=it))


@pytest.mark.parametrize("hot", HOT)
def test_kv_copy_timed_equals_untimed(fa, hot):
    rows, width, sp, dp = 3, 18, 64, 128
    src = np.random.RandomState(6).randint(0, 255, size=(rows, sp), dtype=np.uint8)
    dst = np.full((rows, dp), 0xA5, np.uint8)
    check(fa, hot, 3, ("kv_copy",), lambda it: fa.op_kv_copy(src, dst, width, iters=it))
    want = dst.copy()
    want[:, :width] = src[:, :width]
    assert np.array_equal(_untimed[("kv_copy",)], want)
