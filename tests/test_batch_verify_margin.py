"""CPU part of the fp32 claim of tests/test_gpu_batch_verify.py: in fp32 a member of a packed verify step must accept exactly up to the
planted wrong id, unless a row's top-two gap is below 1e-3, and at most 1 row in 20 may need that.  Here the CPU oracle checks, before
any GPU run, that the chosen packs and prompt seeds stay within that cap: on the oracle's own continuation the rows that decide the
accepted counts keep a top-two gap of 2e-3 (twice the bar, once for each path), the few that do not are at most 1 in 20.  The packs
and seeds are defined here and imported by the GPU test."""
import numpy as np

import synth
from oracle import oracle

MODELS = ["llama_a", "mistral_a", "qwen2_a", "llama_mha", "llama_d100"]   # (test_gpu_verify.py's)
CAP = 96
RAGGED = [(5, 0), (37, 7), (20, 15)]                               # (cached length, drafts) per member
FULL = [(5 + i % 30, 15) for i in range(64)]                       # 64 members x 16 rows = 1024 rows
SEED0 = 1234


def planted(d):
    """where half_right (test_gpu_verify.py) puts the wrong id: what a member accepts when every row is the decode step's"""
    return d // 2 if d >= 7 else d


def oracle_margin(name, spec):
    """(rows of the oracle's own fp32 continuation whose top-two gap is below 2e-3, rows of the pack)"""
    cfg = synth.CONFIGS[name]
    om = oracle.OracleModel(cfg, synth.as_f32(synth.synth_weights(cfg)))
    close, rows = 0, 0
    for i, (L, d) in enumerate(spec):
        _, lg = om.generate(om.new_cache(CAP), synth.prompt_ids(cfg, L, seed=SEED0 + i), planted(d) + 2, want_logits=True)
        s = np.sort(lg, axis=1)
        close += int(((s[:, -1] - s[:, -2]) < 2e-3).sum())
        rows += d + 1
    return close, rows


def test_seeds_keep_the_fp32_margin():
    for name in MODELS:
        close, rows = oracle_margin(name, RAGGED)
        assert close * 20 <= rows, (name, close, rows)
    close, rows = oracle_margin("llama_a", FULL)
    assert close * 20 <= rows, (close, rows)
