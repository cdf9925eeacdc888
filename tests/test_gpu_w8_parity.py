"""The FP8 decode mode (decode_weights="e4m3") at model level.  An FP8 model IS the bf16 model whose weights are W' = s * q
(tests/test_w8_abi.py restates the quantiser on the CPU), so the bar is that bf16 model -- not a quality judgement of the format.

On the nine small configs of tests/test_gpu_parity_bf16.py, teacher-forced with the golden tokens (a prefill on the bf16 image, then
decode steps on the FP8 kernel):
    ref  = oracle(W', fp32)          cand = oracle(W', round_bf16 = 2)
    g16  = Model(W', bf16)           g8   = Model(W, bf16, decode_weights="e4m3")
distances relative L2 over all rows, e_x = d(x, ref)."""
import json
import os

import numpy as np
import pytest

import synth
from oracle import oracle
from test_gpu_parity_bf16 import CASES, rows
from test_w8_abi import dequantized_weights

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def fa():
    import fastllm_amd
    assert fastllm_amd.device_count() >= 1
    return fastllm_amd


_RUNS = {}


def run_case(fa, name, golden_dir):
    if name not in _RUNS:
        z = np.load(os.path.join(golden_dir, name + ".npz"))
        meta = json.loads(bytes(z["meta"]).decode())
        cfg = synth.CONFIGS[name]
        w = synth.synth_weights(cfg)
        wp = dequantized_weights(w)
        g8, g16 = fa.Model(cfg, w, dtype="bf16", decode_weights="e4m3"), fa.Model(cfg, wp, dtype="bf16")
        out = dict(ref=rows(oracle.OracleModel(cfg, synth.as_f32(wp)), z, meta), cand=rows(oracle.OracleModel(cfg, synth.as_f32(wp), round_bf16=2), z, meta),
                   g8=rows(g8, z, meta), g16=rows(g16, z, meta))
        out["prefill8"] = g8.forward(g8.new_cache(64), z["prompt"], 0)
        out["prefill16"] = g16.forward(g16.new_cache(64), z["prompt"], 0)
        g8.close(); g16.close()
        _RUNS[name] = out
    return _RUNS[name]


@pytest.mark.parametrize("name", CASES)
def test_fp8_decode_is_the_bf16_model_of_its_own_weights(fa, name, golden_dir):
    r = run_case(fa, name, golden_dir)
    ref, cand, g8, g16 = r["ref"], r["cand"], r["g8"], r["g16"]
    n = np.linalg.norm(ref)
    e_g8, e_g16, e_cand = (np.linalg.norm(a - ref) / n for a in (g8, g16, cand))
    d = np.linalg.norm(g8 - g16) / n
    print("\n%s: rel L2 to fp32 on W' -- fp8 decode %.3e, bf16 %.3e, candle-emulated bf16 %.3e; fp8 vs bf16 %.3e" % (name, e_g8, e_g16, e_cand, d))
    # 1. no further from the truth on its own weights than the bf16 path on the same weights (they differ in fp32 summation order only;
    #    1.5x and the 1e-4 floor: what test_gpu_parity_bf16.py gives two bf16 executions of one model)
    assert e_g8 <= 1.5 * e_g16 + 1e-4, (e_g8, e_g16)
    # 2. within the reference run's own bf16 noise of the bf16 model
    assert d <= 1.5 * e_cand + 1e-4, (d, e_cand)
    # 4. the prompt's logits are IDENTICAL: same kernels on the same bf16 weights -- the image is W'
    assert np.array_equal(r["prefill8"], r["prefill16"]), np.abs(r["prefill8"] - r["prefill16"]).max()
    assert np.array_equal(g8[0], g16[0])


def test_fp8_greedy_ids_agree_wherever_fp32_decides(fa, golden_dir):
    """3. greedy ids of g8, g16 and ref agree at every step where ref's top-2 margin exceeds 4x the largest max-abs deviation of g8, g16
    and cand from ref; pooled over the nine fixtures (113 steps) at most two thirds of the steps may be left undecided.  (With cand
    alone setting the threshold, on the CPU: 47 of 113 undecided; the synthetic weights give thin logit margins, mistral_win is a
    single undecided step -- hence the pool.)"""
    total = undecided = 0
    for name in CASES:
        r = run_case(fa, name, golden_dir)
        ref = r["ref"]
        top2 = np.sort(ref, axis=1)[:, -2:]
        thr = 4 * max(np.abs(r[k] - ref).max() for k in ("g8", "g16", "cand"))
        decided = (top2[:, 1] - top2[:, 0]) > thr
        total += len(decided)
        undecided += int((~decided).sum())
        print("%s: %d of %d steps undecided (threshold %.3e)" % (name, int((~decided).sum()), len(decided), thr))
        for k in ("g8", "g16"):
            assert (r[k].argmax(1)[decided] == ref.argmax(1)[decided]).all(), (name, k)
    print("pooled: %d of %d steps undecided" % (undecided, total))
    assert total == 113
    assert 3 * undecided <= 2 * total, (undecided, total)


@pytest.mark.parametrize("name", ["llama_a", "qwen2_a", "mistral_d48"])
def test_fp8_captured_loops_and_batches(fa, name):
    """5. fl_decode_greedy / fl_decode_sample (the graph-captured loop) on g8 give the tokens of the step-by-step fl_forward_argmax /
    fl_forward_sample loop on g8; a Batch over caches prefilled on g8 gives the tokens of a Batch on g16 exactly (batches run the
    bf16 kernels on the image)."""
    cfg = synth.CONFIGS[name]
    w = synth.synth_weights(cfg)
    g8, g16 = fa.Model(cfg, w, dtype="bf16", decode_weights="e4m3"), fa.Model(cfg, dequantized_weights(w), dtype="bf16")
    ids = synth.prompt_ids(cfg, 9)
    n = 12
    # greedy
    c = g8.new_cache(64)
    first = g8.forward_argmax(c, ids, 0)
    loop = g8.decode_greedy(c, first, len(ids), n)
    c2 = g8.new_cache(64)
    tok = g8.forward_argmax(c2, ids, 0)
    assert tok == first
    steps = []
    for i in range(n):
        tok = g8.forward_argmax(c2, [tok], len(ids) + i)
        steps.append(tok)
    np.testing.assert_array_equal(loop, np.array(steps, dtype=np.uint32))
    # sampled
    c3, c4 = g8.new_cache(64), g8.new_cache(64)
    f3 = g8.forward_sample(c3, ids, 0, 0.8, seed=3)
    loop = g8.decode_sample(c3, f3, len(ids), n, 0.8, seed=3, draws_done=1)
    tok = g8.forward_sample(c4, ids, 0, 0.8, seed=3)
    steps = []
    for i in range(n):
        tok = g8.forward_sample(c4, [tok], len(ids) + i, 0.8, seed=3, draws_done=1 + i)
        steps.append(tok)
    np.testing.assert_array_equal(loop, np.array(steps, dtype=np.uint32))
    # batch
    out = []
    for m in (g8, g16):
        ca, cb = m.new_cache(64), m.new_cache(64)
        fa_, fb_ = m.forward_argmax(ca, ids, 0), m.forward_argmax(cb, ids[:5], 0)
        out.append((fa_, fb_, fa.Batch(m, [ca, cb]).decode([fa_, fb_], [len(ids), 5], 8)))
    assert out[0][:2] == out[1][:2]
    for a, b in zip(out[0][2], out[1][2]):
        np.testing.assert_array_equal(a, b)
    g8.close(); g16.close()


def test_fp8_info_and_short_cache(fa):
    """6. info(): decode_weights, the bytes the FP8 step streams (1 per projection weight + 4 per projection row), both images
    allocated; a bf16 model's info is what it was; a cache short enough for the replicated-attention launch on a bf16 model decodes
    correctly on g8 (which does not take that launch)."""
    cfg = synth.CONFIGS["mistral_a"]
    w = synth.synth_weights(cfg)
    wp = dequantized_weights(w)
    g8, g16 = fa.Model(cfg, w, dtype="bf16", decode_weights="e4m3"), fa.Model(cfg, wp, dtype="bf16")
    i8, i16 = g8.info(), g16.info()
    h, I, V, L = cfg["hidden_size"], cfg["intermediate_size"], cfg["vocab_size"], cfg["num_hidden_layers"]
    H, Hkv = cfg["num_attention_heads"], cfg["num_key_value_heads"]
    d = h // H
    proj_w = L * (2 * h * h + 2 * Hkv * d * h + 3 * h * I) + V * h
    proj_rows = L * (h + 2 * Hkv * d + h + 2 * I + h) + V
    small = L * 2 * h + h                                   # norms and the embedding row, counted at the compute dtype as before
    assert i16.decode_weights == 0 and i16.weight_bytes_per_token == 2 * (proj_w + small)
    assert i8.decode_weights == 1 and i8.weight_bytes_per_token == proj_w + 4 * proj_rows + 2 * small
    assert i8.hbm_bytes_allocated >= i16.hbm_bytes_allocated + proj_w + 4 * proj_rows          # 1.5x the weights: both images
    assert i8.compute_dtype == i16.compute_dtype == 1 and i8.kv_bytes_per_position == i16.kv_bytes_per_position
    plain = fa.Model(cfg, wp, dtype="bf16", decode_weights="compute").info()
    for f, _ in type(plain)._fields_:
        if f != "cfg":
            assert getattr(plain, f) == getattr(i16, f), f
    ids = synth.prompt_ids(cfg, 6)
    # the FP8 model's decode step runs the FP8 kernel for all six projections (4 launches per layer + lm_head; o_proj is a launch of
    # its own: no replicated attention), the bf16 model's none
    for m, want in ((g8, True), (g16, False)):
        c = m.new_cache(16)
        tok = m.forward_argmax(c, ids, 0)
        m.profile_begin()
        m.forward_argmax(c, [tok], len(ids))
        names = {s["name"]: s["launches"] for s in m.profile_end()}
        w8 = sum(v for k, v in names.items() if k.startswith("gemv") and ",w8]" in k)
        other = sum(v for k, v in names.items() if k.startswith("gemv") and ",w8]" not in k)
        assert (w8, other) == ((4 * L + 1, 0) if want else (0, other)), names
        assert want or other >= 3 * L + 1, names
        c.close()
    got = []
    for m in (g8, g16):
        c = m.new_cache(16)                                 # (short: the bf16 model's decode takes the replicated-attention launch)
        lg = [m.forward(c, ids, 0)]
        for i in range(4):
            lg.append(m.forward(c, [int(np.argmax(lg[0])) if i == 0 else 7 + i], len(ids) + i))
        got.append(np.stack(lg))
    assert np.array_equal(got[0][0], got[1][0])
    nrm = np.linalg.norm(got[1])
    assert np.linalg.norm(got[0] - got[1]) <= 1e-2 * nrm, np.linalg.norm(got[0] - got[1]) / nrm      # (bf16 noise floor between two kernel paths of this suite)
    g8.close(); g16.close()
