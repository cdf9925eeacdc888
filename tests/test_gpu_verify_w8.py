"""The verify step of an FP8 model (decode_weights="e4m3") reads the e4m3 bytes (k_gemm_rows_w8.hip; fl_tune "verify_w8").  An FP8
model IS the bf16 model of W' = s * q (tests/test_gpu_w8_parity.py): with the switch off the step's rows are that model's bit for bit;
with it on they differ in fp32 summation order only, and are held to the rule that file has for two such executions."""
import numpy as np
import pytest

import synth
from oracle import oracle
from test_gpu_verify import expected
from test_w8_abi import dequantized_weights

pytestmark = pytest.mark.gpu
L = 9


@pytest.fixture(scope="module")
def fa():
    import fastllm_amd
    assert fastllm_amd.device_count() >= 1
    return fastllm_amd


@pytest.mark.parametrize("n_draft", [3, 15])
@pytest.mark.parametrize("name", ["mistral_a", "qwen2_a"])
def test_verify_step_streams_the_e4m3_bytes(fa, name, n_draft):
    cfg = synth.CONFIGS[name]
    w = synth.synth_weights(cfg)
    wp = dequantized_weights(w)
    g8, g16 = fa.Model(cfg, w, dtype="bf16", decode_weights="e4m3"), fa.Model(cfg, wp, dtype="bf16")
    om = oracle.OracleModel(cfg, synth.as_f32(wp))
    p = synth.prompt_ids(cfg, L)
    c = g16.new_cache(64)
    first = g16.forward_argmax(c, p, 0)
    draft = np.array(g16.decode_greedy(c, first, L, n_draft), np.uint32)     # the bf16 model's own continuation ...
    draft[n_draft // 2] = (draft[n_draft // 2] + 1) % cfg["vocab_size"]       # ... with a wrong id in the middle

    def step(m, switch):
        fa.tune("verify_w8", switch)
        c = m.new_cache(64)
        assert m.forward_argmax(c, p, 0) == first                           # (the prompt runs on the image in both models)
        toks, lg = m.forward_verify(c, first, draft, L, want_logits=True)
        assert toks.tolist() == expected(lg, draft) and len(c) == L + len(toks)
        return lg

    try:
        on, off, ref16 = step(g8, 1), step(g8, 0), step(g16, 1)
    finally:
        fa.tune("verify_w8", 1)
    oc = om.new_cache(64)
    om.forward(oc, p, 0)
    ref = np.stack([om.forward(oc, [t], L + i) for i, t in enumerate([first] + draft.tolist())])
    assert np.array_equal(off, ref16)                                        # switch 0: the launches of the bf16 image
    assert not np.array_equal(on, off)                                       # switch 1: another kernel, another summation order
    e8, e16 = (np.linalg.norm(a - ref) / np.linalg.norm(ref) for a in (on, ref16))
    print("\n%s n_draft %d: rel L2 to fp32 on W' -- fp8 verify %.3e, bf16 %.3e" % (name, n_draft, e8, e16))
    assert e8 <= 1.5 * e16 + 1e-4, (e8, e16)
    g8.close(); g16.close()
