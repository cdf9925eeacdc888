"""tests/decoder_ref.py anchored to the project's oracle on the CPU: its causal hidden states, projected through lm_head, are the
golden prefill logits (tests/golden/*.npz) and the oracle's logits of a fresh prompt, within 1e-4.  Its full-mask mode differs from
the causal one in the mask alone, so the full-mask reference of tests/test_gpu_embed.py stands on this anchor."""
import os

import numpy as np
import pytest

import decoder_ref
import synth
from oracle import oracle

NAMES = ["llama_a", "mistral_win", "qwen2_win", "llama_mha"]
TOL = 1e-4


@pytest.mark.parametrize("name", NAMES)
def test_causal_hidden_states_give_the_golden_prefill_logits(name, golden_dir):
    z = np.load(os.path.join(golden_dir, name + ".npz"))
    cfg = synth.CONFIGS[name]
    w = synth.as_f32(synth.synth_weights(cfg))
    hid = decoder_ref.hidden_states(cfg, w, z["prompt"])
    got = decoder_ref.logits(cfg, w, hid[-1])
    err = np.abs(got - z["prefill_logits"]).max()
    print("%s: T = %d, max |ref - golden| = %.3g" % (name, len(z["prompt"]), err))
    assert err <= TOL


@pytest.mark.parametrize("name", NAMES)
def test_causal_hidden_states_give_the_oracles_logits_on_a_fresh_prompt(name):
    cfg = synth.CONFIGS[name]
    w = synth.as_f32(synth.synth_weights(cfg))
    ids = synth.prompt_ids(cfg, 23, seed=4711)
    om = oracle.OracleModel(cfg, w)
    hid = decoder_ref.hidden_states(cfg, w, ids)
    for n in (1, 7, 23):                                   # a row's state under the causal mask is that of the prefix that ends there
        want = om.forward(om.new_cache(32), ids[:n], 0)
        err = np.abs(decoder_ref.logits(cfg, w, hid[n - 1]) - want).max()
        print("%s: prefix %d, max |ref - oracle| = %.3g" % (name, n, err))
        assert err <= TOL
    om.close()


def test_full_mask_differs_from_causal_only_where_it_must():
    cfg = synth.CONFIGS["mistral_win"]
    w = synth.as_f32(synth.synth_weights(cfg))
    ids = synth.prompt_ids(cfg, 17, seed=5)
    causal, full = decoder_ref.hidden_states(cfg, w, ids), decoder_ref.hidden_states(cfg, w, ids, mask="full")
    assert np.abs(causal[0] - full[0]).max() > 1e-3        # row 0 sees 16 more keys
    # one token: both masks see the one key
    assert np.array_equal(decoder_ref.hidden_states(cfg, w, ids[:1]), decoder_ref.hidden_states(cfg, w, ids[:1], mask="full"))
    # the full mask ignores the window: the same model without one gives the same states
    nowin = dict(cfg, sliding_window=None)
    assert np.array_equal(full, decoder_ref.hidden_states(nowin, w, ids, mask="full"))
    assert decoder_ref.visible(4, "causal", 1).tolist() == [[True, False, False, False], [True, True, False, False],
                                                            [False, True, True, False], [False, False, True, True]]


def test_pooling_restatement():
    hid = np.arange(12, dtype=np.float32).reshape(4, 3)
    assert decoder_ref.pool_f32(hid, [1, 3], "last").tolist() == [[0, 1, 2], [9, 10, 11]]
    assert decoder_ref.pool_f32(hid, [1, 3], "first", dims=2).tolist() == [[0, 1], [3, 4]]
    assert decoder_ref.pool_f32(hid, [1, 3], "mean").tolist() == [[0, 1, 2], [6, 7, 8]]
    assert decoder_ref.pool_f32(hid, [1, 3], "none", dims=1).tolist() == [[0], [3], [6], [9]]
    n = decoder_ref.normalize_f64(np.array([[3.0, 4.0], [0.0, 0.0]], np.float32))
    assert n.tolist() == [[0.6, 0.8], [0.0, 0.0]]
