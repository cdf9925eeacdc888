"""The three bf16 MFMA attention kernels (decode, 16-row prefill, 32-row prefill) ALONE, through fl_op_attention,
against an fp64 numpy reference: head_dim 64 / 128, GQA group sizes 1 / 4 / 7 / 8, key counts that straddle the decode
kernel's split boundaries (128 keys per split), tile boundaries (32 keys) and the sliding window.  VERDICT r01 item 5c:
these kernels were otherwise only seen through whole-model logits at a 1-2 % tolerance."""
import numpy as np
import pytest

import synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fa():
    import fastllm_amd
    assert fastllm_amd.device_count() >= 1
    return fastllm_amd


def make(T, s_past, H, Hkv, d, seed, spike=False):
    rs = np.random.RandomState(seed)
    q = synth.f32_to_bf16_bits(rs.standard_normal((T, H * d)).astype(np.float32))
    k = synth.f32_to_bf16_bits(rs.standard_normal((s_past + T, Hkv * d)).astype(np.float32))
    v = synth.f32_to_bf16_bits(rs.standard_normal((s_past + T, Hkv * d)).astype(np.float32))
    if spike:
        # one key far above the rest late in the sequence: the running max jumps there, every earlier partial sum must be
        # rescaled (the rare branch of an online softmax; cdna guide rule 26)
        kk = synth.bf16_bits_to_f32(k).reshape(s_past + T, Hkv, d)
        qq = synth.bf16_bits_to_f32(q).reshape(T, H, d)
        pos = s_past + T - 3 if T > 3 else max(0, s_past - 5)
        kk[pos, :, :] = 4.0 * qq[-1].reshape(Hkv, H // Hkv, d)[:, 0, :] / np.sqrt(d) * 3
        k = synth.f32_to_bf16_bits(kk.reshape(s_past + T, Hkv * d))
    return q, k, v


def reference(q, k, v, s_past, H, Hkv, d, window, call0=None, dtype=np.float64):
    """q, k, v: bf16 bits (uint16) or float arrays.  call0 (default s_past): the cached length when the API call began; below s_past
    it is the mask of a later chunk of a prefill cut into chunks: keys before call0 are visible, key j >= call0 is visible to the
    query at position p iff j <= p and j + window >= p.  dtype: the precision the whole computation runs in."""
    def wide(a):
        a = np.asarray(a)
        return (synth.bf16_bits_to_f32(a) if a.dtype == np.uint16 else a).astype(dtype)
    qf, kf, vf = wide(q).reshape(-1, H, d), wide(k).reshape(-1, Hkv, d), wide(v).reshape(-1, Hkv, d)
    T, S, G = qf.shape[0], kf.shape[0], H // Hkv
    c0 = s_past if call0 is None else call0
    out = np.zeros((T, H, d), dtype=dtype)
    for h in range(H):
        g = h // G                                               # App. A.6: q head h uses kv head h // (H / Hkv)
        sc = qf[:, h, :] @ kf[:, g, :].T / np.sqrt(dtype(d))     # [T, S]
        if T > 1:                                                # App. A.5: no mask at T == 1
            p = s_past + np.arange(T)[:, None]
            j = np.arange(S)[None, :]
            vis = (j < c0) | ((j <= p) & ((window < 0) | (j + window >= p)))
            sc = np.where(vis, sc, -np.inf)
        sc -= sc.max(axis=1, keepdims=True)
        p = np.exp(sc)
        p /= p.sum(axis=1, keepdims=True)
        out[:, h, :] = p @ vf[:, g, :]
    return out.reshape(T, H * d)


def check(got, ref, what):
    assert np.isfinite(got).all(), what + ": non-finite output (an element the kernel did not write?)"
    err = np.abs(got - ref)
    scale = max(1e-6, np.abs(ref).max())
    rel = np.linalg.norm(got - ref) / max(1e-30, np.linalg.norm(ref))
    # P is rounded to bf16 before P.V and the output is bf16: 2^-9 relative per rounding, averaged over the keys
    assert err.max() <= 1.2e-2 * scale and rel <= 5e-3, "%s: max err %.3g (scale %.3g), rel L2 %.2e" % (what, err.max(), scale, rel)


GROUPS = [(8, 8), (32, 8), (28, 4), (8, 1)]                      # (H, Hkv): G = 1, 4, 7, 8


@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("H,Hkv", GROUPS)
@pytest.mark.parametrize("S,nsplit", [(1, 1), (31, 1), (127, 1), (128, 1), (129, 2), (300, 0), (640, 0), (1025, 0), (1025, 1), (2500, 48),
                                      (1025, 2), (2048, 4), (4100, 17), (4100, 34)])   # 4-wave splits of 2 / 4 / 4 / 2 (256-key) steps per wave: the long-cache rule
def test_decode_kernel(fa, d, H, Hkv, S, nsplit):
    q, k, v = make(1, S - 1, H, Hkv, d, seed=S * 7 + d + H)
    got = fa.op_attention(q, k, v, S - 1, H, Hkv, d, kernel=1, nsplit=nsplit)
    check(got, reference(q, k, v, S - 1, H, Hkv, d, -1), "decode d=%d G=%d S=%d nsplit=%d" % (d, H // Hkv, S, nsplit))


PREFILL_CASES = [(2, 0, -1), (16, 0, -1), (33, 0, -1), (100, 0, 5), (130, 0, 32), (257, 0, -1), (64, 40, -1), (70, 129, 17)]   # (T, s_past, window)


def prefill_inputs(T, s_past, H, Hkv, d, kernel):
    """q, k, v of one test_prefill_kernels case (tools/output_digests.py runs the same cases)"""
    return make(T, s_past, H, Hkv, d, seed=T * 3 + s_past + d + H + kernel)


@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("H,Hkv", GROUPS)
@pytest.mark.parametrize("kernel", [2, 3])
@pytest.mark.parametrize("T,s_past,window", PREFILL_CASES)
def test_prefill_kernels(fa, d, H, Hkv, kernel, T, s_past, window):
    q, k, v = prefill_inputs(T, s_past, H, Hkv, d, kernel)
    got = fa.op_attention(q, k, v, s_past, H, Hkv, d, window=window, kernel=kernel)
    check(got, reference(q, k, v, s_past, H, Hkv, d, window), "prefill%d d=%d G=%d T=%d past=%d w=%d" % (kernel, d, H // Hkv, T, s_past, window))


@pytest.mark.parametrize("d,H,Hkv", [(128, 32, 8), (64, 32, 4), (128, 28, 4)])          # Mistral-7B, TinyLlama, Qwen2-7B head shapes
def test_baseline_shapes_and_the_rescale_branch(fa, d, H, Hkv):
    # decode at S = 640 (the bench's kv length) with a late spike; long prefill on both kernels with a window that bites
    q, k, v = make(1, 639, H, Hkv, d, seed=5, spike=True)
    check(fa.op_attention(q, k, v, 639, H, Hkv, d, kernel=1), reference(q, k, v, 639, H, Hkv, d, -1), "decode spike")
    q, k, v = make(1100, 0, H, Hkv, d, seed=6, spike=True)
    for kernel in (2, 3):
        check(fa.op_attention(q, k, v, 0, H, Hkv, d, window=300, kernel=kernel), reference(q, k, v, 0, H, Hkv, d, 300),
              "prefill%d spike window" % kernel)
    # kernel = 0: what the model would launch at this length
    check(fa.op_attention(q, k, v, 0, H, Hkv, d, window=-1, kernel=0), reference(q, k, v, 0, H, Hkv, d, -1), "prefill auto")


@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("H,Hkv", [(8, 8), (8, 4), (32, 8), (28, 4), (8, 1), (10, 2)])    # G = 1, 2, 4: wave pairs fit; 7, 8, 5: dealt as subgroups of 4 heads
@pytest.mark.parametrize("T,s_past,window", [(33, 0, -1), (100, 0, 5), (257, 0, -1), (70, 129, 17), (1100, 0, 300), (2100, 0, -1)])
def test_prefill32_key_split(fa, monkeypatch, d, H, Hkv, T, s_past, window):
    """KS2: two waves per (head, 32-token block) on alternate key tiles, merged through LDS (what prompts of ~1-4 k tokens
    get when there are too few blocks to balance): odd and even tile counts, a single tile, cached prefix, window, a ragged
    last block; T = 2100 with 8 kv heads is 528 items: the snake's second round as well.  Then the same with FOUR waves per
    (head, block) on every fourth key tile (two ring slots of four tiles, groups of >= 4 heads dealt two heads at a time,
    three partners merged in key-tile order): tile counts 1 .. 3 below the wave count leave partner waves without a tile."""
    if T > 2000 and (H, Hkv) not in ((32, 8), (28, 4)):
        pytest.skip("the 2100-token case (the snake's second round) runs on the two benchmark head layouts: its numpy reference is 3.5 s a case")
    q, k, v = make(T, s_past, H, Hkv, d, seed=T + s_past + d + H, spike=T > 1000)
    ref = reference(q, k, v, s_past, H, Hkv, d, window)
    for ks in (1, 4):
        monkeypatch.setenv("FL_ATTN_PF32_KS2", str(ks))
        got = fa.op_attention(q, k, v, s_past, H, Hkv, d, window=window, kernel=3)
        check(got, ref, "prefill32 ks%d d=%d G=%d T=%d past=%d w=%d" % (2 if ks == 1 else 4, d, H // Hkv, T, s_past, window))


_SCHED_REF = {}


@pytest.mark.parametrize("d,H,Hkv", [(128, 32, 8), (128, 28, 4)])
@pytest.mark.parametrize("sched", [0, 1, 2])
def test_prefill32_schedules(fa, monkeypatch, d, H, Hkv, sched):
    """The 32-row kernel's three work distributions -- plain (long blocks first), paired, snake (persistent workgroups; what
    long prompts get) -- on a prompt whose (block, kv head) items exceed one round of the chip (264 > 256: some workgroups take
    two), with a ragged last block (2100 % 32 = 20) and a window that bites."""
    monkeypatch.setenv("FL_ATTN_PF32_PAIRED", str(sched))
    monkeypatch.setenv("FL_ATTN_PF32_KS2", "0")
    T = 2100
    q, k, v = make(T, 0, H, Hkv, d, seed=77, spike=True)              # (the same inputs for the three schedules: one numpy reference)
    for window in (-1, 1000):
        got = fa.op_attention(q, k, v, 0, H, Hkv, d, window=window, kernel=3)
        key = (d, H, Hkv, window)
        if key not in _SCHED_REF:
            _SCHED_REF[key] = reference(q, k, v, 0, H, Hkv, d, window)
        check(got, _SCHED_REF[key], "prefill32 schedule %d window %d" % (sched, window))


def test_bad_arguments_are_errors(fa):
    q, k, v = make(2, 0, 8, 8, 64, 1)
    with pytest.raises(fa.FastLLMError):
        fa.op_attention(q, k, v, 0, 8, 8, 64, kernel=1)            # decode kernel with T = 2
    q, k, v = make(1, 3, 18, 2, 64, 1)
    with pytest.raises(fa.FastLLMError):
        fa.op_attention(q, k, v, 3, 18, 2, 64)                     # 9 query heads per kv head
