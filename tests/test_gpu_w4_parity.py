"""An MXFP4 model against the bf16 model of the restatement's image (tests/test_w4_abi.py): bit for bit, but for the T = 1 step's fp32 summation order."""
import numpy as np
import pytest

import synth
from test_gpu_w8_ops import fa  # noqa: F401  (the fixture)
from test_w4_abi import mx4_image_weights

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", params=["llama_a", "mistral_a", "qwen2_a"])                # qwen2_a: q/k/v bias through the RoPE epilogue
def pair(request, fa):
    cfg = synth.CONFIGS[request.param]
    w = synth.synth_weights(cfg)
    g4, g16 = fa.Model(cfg, w, dtype="bf16", decode_weights="mxfp4"), fa.Model(cfg, mx4_image_weights(w), dtype="bf16")
    yield cfg, g4, g16
    g4.close(); g16.close()


def test_prefill_is_identical_and_the_step_agrees(pair):
    cfg, g4, g16 = pair
    ids = synth.prompt_ids(cfg, 9)
    got = []
    for m in (g4, g16):
        c = m.new_cache(64)
        lg = [m.forward(c, ids, 0)]
        for i in range(4):
            lg.append(m.forward(c, [int(np.argmax(lg[0])) if i == 0 else 7 + i], len(ids) + i))
        got.append(np.stack(lg))
    assert np.array_equal(got[0][0], got[1][0]), np.abs(got[0][0] - got[1][0]).max()      # same kernels on the same image
    nrm, d = np.linalg.norm(got[1][1:]), np.linalg.norm(got[0][1:] - got[1][1:])
    assert d <= 1e-2 * nrm, d / nrm                        # (tests/test_gpu_w8_parity.py's bound for the FP8 model against its image)


def test_captured_loop_equals_single_steps(pair):
    cfg, g4, _ = pair
    ids, n = synth.prompt_ids(cfg, 9), 12
    c, c2 = g4.new_cache(64), g4.new_cache(64)
    first, tok = g4.forward_argmax(c, ids, 0), g4.forward_argmax(c2, ids, 0)
    loop = g4.decode_greedy(c, first, len(ids), n)
    steps = []
    for i in range(n):
        steps.append(tok := g4.forward_argmax(c2, [tok], len(ids) + i))
    np.testing.assert_array_equal(loop, np.array(steps, dtype=np.uint32))


def test_batch_and_verify_run_on_the_image(pair, fa):
    cfg, g4, g16 = pair
    ids = synth.prompt_ids(cfg, 9)
    out = []
    for m in (g4, g16):
        ca, cb, cv = m.new_cache(64), m.new_cache(64), m.new_cache(64)
        ta, tb = m.forward_argmax(ca, ids, 0), m.forward_argmax(cb, ids[:5], 0)
        batch = fa.Batch(m, [ca, cb]).decode([ta, tb], [len(ids), 5], 8)
        tv = m.forward_argmax(cv, ids, 0)
        toks, lg = m.forward_verify(cv, tv, [3, 5, 7], len(ids), want_logits=True)       # a verify step of 4 rows
        out.append((ta, tb, [np.asarray(b) for b in batch], tv, np.asarray(toks), lg))
    assert out[0][:2] == out[1][:2] and out[0][3] == out[1][3]
    for a, b in zip(out[0][2] + list(out[0][4:]), out[1][2] + list(out[1][4:])):     # the batch's streams, the verify step's ids and rows
        np.testing.assert_array_equal(a, b)


def test_info_reports_the_format_and_its_bytes(pair):
    cfg, g4, g16 = pair
    i4, i16 = g4.info(), g16.info()
    h, I, V, L = cfg["hidden_size"], cfg["intermediate_size"], cfg["vocab_size"], cfg["num_hidden_layers"]
    Hkv, d = cfg["num_key_value_heads"], h // cfg["num_attention_heads"]
    proj_w = L * (2 * h * h + 2 * Hkv * d * h + 3 * h * I) + V * h
    small = L * (2 * h + (h + 2 * Hkv * d if cfg.get("qkv_bias") else 0)) + h   # norms, biases and the embedding row, at the compute dtype as before
    assert i16.decode_weights == 0 and i16.weight_bytes_per_token == 2 * (proj_w + small)
    assert i4.decode_weights == 2 and i4.weight_bytes_per_token == proj_w // 2 + proj_w // 32 + 2 * small
    assert i4.hbm_bytes_allocated >= i16.hbm_bytes_allocated + proj_w // 2 + proj_w // 32        # nibbles, scales AND the image
    ids = synth.prompt_ids(cfg, 6)
    c = g4.new_cache(16)
    tok = g4.forward_argmax(c, ids, 0)
    g4.profile_begin()
    g4.forward_argmax(c, [tok], len(ids))
    names = {s["name"]: s["launches"] for s in g4.profile_end()}
    w4 = sum(v for k, v in names.items() if k.startswith("gemv") and ",w4]" in k)
    other = sum(v for k, v in names.items() if k.startswith("gemv") and ",w4]" not in k)
    assert (w4, other) == (4 * L + 1, 0), names      # the T = 1 step: the MXFP4 kernel for all six projections, no other weight stream
