"""A decode batch of 3-64 members on an FP8 model (decode_weights="e4m3") reads the e4m3 bytes (k_gemm_rows_w8.hip up to 16 members,
k_gemm_rows64_w8.hip from 17; fl_tune "batch_w8", read when the Batch is created).  An FP8 model IS the bf16 model of W' = s * q
(tests/test_gpu_w8_parity.py): with the switch off the step's rows are that model's bit for bit; with it on they differ in fp32
summation order only, and are held to the rule that file has for two such executions."""
import numpy as np
import pytest

import synth
from oracle import oracle
from test_w8_abi import dequantized_weights

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fa():
    import fastllm_amd
    assert fastllm_amd.device_count() >= 1
    return fastllm_amd


def prompt(cfg, i):
    return synth.prompt_ids(cfg, 3 + i % 5, seed=1234 + i)


def rel(a, ref):
    return np.linalg.norm(a - ref) / np.linalg.norm(ref)


def members(m, cfg, idx):
    """a cache per member, prefilled with its own prompt (on the image in both models): caches, first tokens, positions"""
    caches = [m.new_cache(64) for _ in idx]
    return caches, [m.forward_argmax(c, prompt(cfg, i), 0) for c, i in zip(caches, idx)], [len(prompt(cfg, i)) for i in idx]


def oracle_row(om, cfg, i, tok):
    oc = om.new_cache(64)
    om.forward(oc, prompt(cfg, i), 0)
    return om.forward(oc, [tok], len(prompt(cfg, i)))


@pytest.mark.parametrize("B", [3, 17, 33])
@pytest.mark.parametrize("name", ["mistral_a", "qwen2_a"])
def test_batch_step_streams_the_e4m3_bytes(fa, name, B):
    cfg = synth.CONFIGS[name]
    w = synth.synth_weights(cfg)
    wp = dequantized_weights(w)
    g8, g16 = fa.Model(cfg, w, dtype="bf16", decode_weights="e4m3"), fa.Model(cfg, wp, dtype="bf16")
    om = oracle.OracleModel(cfg, synth.as_f32(wp))

    def step(m, switch):
        fa.tune("batch_w8", switch)
        caches, toks, pos = members(m, cfg, range(B))
        lg, _ = fa.Batch(m, caches).forward(toks, pos, want_logits=True)       # (created after the tune call: the switch is read there)
        assert [len(c) for c in caches] == [p + 1 for p in pos]
        return lg, toks

    try:
        (on, toks), (off, toks_off), (ref16, toks16) = step(g8, 1), step(g8, 0), step(g16, 1)
    finally:
        fa.tune("batch_w8", 1)
    assert toks == toks_off == toks16
    ref = np.stack([oracle_row(om, cfg, i, t) for i, t in enumerate(toks)])
    assert np.array_equal(off, ref16)                                        # switch 0: the launches of the bf16 image
    assert not np.array_equal(on, off)                                       # switch 1: other kernels, another summation order
    e8, e16 = rel(on, ref), rel(ref16, ref)
    print("\n%s B %d: rel L2 to fp32 on W' -- fp8 batch %.3e, bf16 %.3e" % (name, B, e8, e16))
    assert e8 <= 1.5 * e16 + 1e-4, (e8, e16)
    g8.close(); g16.close()


def test_replaced_member_streams_them_too(fa):
    """fl_batch_replace on a 17-member FP8 batch, then a second step: the new member's row against the same step of the bf16 model."""
    cfg, B, slot, new = synth.CONFIGS["mistral_a"], 17, 5, 40
    w = synth.synth_weights(cfg)
    wp = dequantized_weights(w)
    g8, g16 = fa.Model(cfg, w, dtype="bf16", decode_weights="e4m3"), fa.Model(cfg, wp, dtype="bf16")
    rows = []
    for m in (g8, g16):
        caches, toks, pos = members(m, cfg, range(B))
        b = fa.Batch(m, caches)
        _, nxt = b.forward(toks, pos, want_logits=True)
        (c,), (t,), (p,) = members(m, cfg, [new])
        b.replace(slot, c)
        toks2, pos2 = nxt.tolist(), [q + 1 for q in pos]
        toks2[slot], pos2[slot] = t, p
        rows.append(b.forward(toks2, pos2, want_logits=True)[0][slot])
        assert len(c) == p + 1
    ref = oracle_row(oracle.OracleModel(cfg, synth.as_f32(wp)), cfg, new, t)
    e8, e16 = rel(rows[0], ref), rel(rows[1], ref)
    assert not np.array_equal(rows[0], rows[1])
    assert e8 <= 1.5 * e16 + 1e-4, (e8, e16)
    g8.close(); g16.close()
