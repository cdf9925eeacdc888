"""Verify steps and batches of 3-16 members of an MXFP4 model (decode_weights="mxfp4") under fl_tune "rows_w4" read the e2m1 nibbles
(k_gemm_rows_w4.hip).  An MXFP4 model IS the bf16 model of W' = 2^e * q (tests/test_gpu_w4_parity.py): with the switch off (the
default) the rows are that model's bit for bit; with it on they differ in fp32 summation order only, and are held to the rule
tests/test_gpu_verify_w8.py and tests/test_gpu_batch_w8.py have for two such executions."""
import numpy as np
import pytest

import synth
from oracle import oracle
from test_gpu_batch_w8 import members, oracle_row, rel
from test_gpu_verify import expected
from test_w4_abi import mx4_image_weights

pytestmark = pytest.mark.gpu
L = 9


@pytest.fixture(scope="module")
def fa():
    import fastllm_amd
    assert fastllm_amd.device_count() >= 1
    return fastllm_amd


def models(fa, name):
    cfg = synth.CONFIGS[name]
    w = synth.synth_weights(cfg)
    wp = mx4_image_weights(w)
    return cfg, fa.Model(cfg, w, dtype="bf16", decode_weights="mxfp4"), fa.Model(cfg, wp, dtype="bf16"), oracle.OracleModel(cfg, synth.as_f32(wp))


def w4_launches(m, run):
    m.profile_begin()
    out = run()
    return out, sum(s["launches"] for s in m.profile_end() if "[rows" in s["name"] and ",w4]" in s["name"])


@pytest.mark.parametrize("n_draft", [3, 15])
@pytest.mark.parametrize("name", ["mistral_a", "qwen2_a"])
def test_verify_step_streams_the_nibbles(fa, name, n_draft):
    cfg, g4, g16, om = models(fa, name)
    p = synth.prompt_ids(cfg, L)
    c = g16.new_cache(64)
    first = g16.forward_argmax(c, p, 0)
    draft = np.array(g16.decode_greedy(c, first, L, n_draft), np.uint32)     # the bf16 model's own continuation ...
    draft[n_draft // 2] = (draft[n_draft // 2] + 1) % cfg["vocab_size"]       # ... with a wrong id in the middle

    def step(m, switch):
        fa.tune("rows_w4", switch)
        c = m.new_cache(64)
        assert m.forward_argmax(c, p, 0) == first                           # (the prompt runs on the image in both models)
        (toks, lg), n_w4 = w4_launches(m, lambda: m.forward_verify(c, first, draft, L, want_logits=True))
        assert toks.tolist() == expected(lg, draft) and len(c) == L + len(toks)
        return lg, n_w4

    try:
        (on, n_on), (off, n_off), (ref16, _) = step(g4, 1), step(g4, 0), step(g16, 1)
    finally:
        fa.tune("rows_w4", 0)
    oc = om.new_cache(64)
    om.forward(oc, p, 0)
    ref = np.stack([om.forward(oc, [t], L + i) for i, t in enumerate([first] + draft.tolist())])
    assert np.array_equal(off, ref16) and n_off == 0                         # switch 0: the launches of the bf16 image
    assert not np.array_equal(on, off) and n_on > 0                          # switch 1: another kernel, another summation order
    e4, e16 = rel(on, ref), rel(ref16, ref)
    print("\n%s n_draft %d: rel L2 to fp32 on W' -- mxfp4 verify %.3e, bf16 %.3e, %d w4 launches" % (name, n_draft, e4, e16, n_on))
    assert e4 <= 1.5 * e16 + 1e-4, (e4, e16)
    g4.close(); g16.close()


@pytest.mark.parametrize("B", [3, 16])
def test_batch_step_streams_the_nibbles(fa, B):
    cfg, g4, g16, om = models(fa, "mistral_a")

    def step(m, switch):
        fa.tune("rows_w4", switch)
        caches, toks, pos = members(m, cfg, range(B))
        b = fa.Batch(m, caches)                                             # (created after the tune call: the switch is read there)
        (lg, _), n_w4 = w4_launches(m, lambda: b.forward(toks, pos, want_logits=True))
        assert [len(c) for c in caches] == [p + 1 for p in pos]
        return lg, toks, n_w4

    try:
        (on, toks, n_on), (off, toks_off, n_off), (ref16, toks16, _) = step(g4, 1), step(g4, 0), step(g16, 1)
    finally:
        fa.tune("rows_w4", 0)
    assert toks == toks_off == toks16
    ref = np.stack([oracle_row(om, cfg, i, t) for i, t in enumerate(toks)])
    assert np.array_equal(off, ref16) and n_off == 0
    assert not np.array_equal(on, off) and n_on > 0
    e4, e16 = rel(on, ref), rel(ref16, ref)
    print("\nB %d: rel L2 to fp32 on W' -- mxfp4 batch %.3e, bf16 %.3e, %d w4 launches" % (B, e4, e16, n_on))
    assert e4 <= 1.5 * e16 + 1e-4, (e4, e16)
    g4.close(); g16.close()
