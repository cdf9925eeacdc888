"""What logit rules (logit_bias + repetition / frequency / presence penalties, fl_cache_set_logit_rules) cost a decode loop, measured
in ONE process on Mistral-7B-shaped random weights in bf16.

Four settings interleaved round by round (so drift hits them alike), the order reversed every other round: greedy with rules off --
fl_decode_greedy, the step every earlier commit runs and the yardstick here -- greedy with rules on, and the same pair under
temperature 0.8 / top-p 0.9 sampling.  Every sample is K graph-replayed steps on a cache of its own -- so each side captures its
graph afresh -- behind 16 warm-up steps; reported: median tokens/s with the min .. max spread over the rounds.

With rules on a step has one more launch (logit_rules_kernel: V x 16 bytes, mostly from L2), and a greedy step's ArgMax reads the
whole adjusted row instead of the lm_head launch's per-workgroup candidates.

Then the kernel alone: its launches inside real decode steps, bracketed by events (fl_profile_*; "select_advance[rules]"), at
V = 32 000 (the 7B model above) and V = 152 064 (a two-layer model with that vocabulary: the launch only sees the logits row).

    python tools/logit_rules_cost.py [--prompt 512] [--steps 256] [--rounds 7]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402  (first: its HIP runtime must initialise before the product library's, as in bench.py)
import bench  # noqa: E402
import fastllm_amd as fa  # noqa: E402
from fastllm_amd.configs import MODEL_CONFIGS  # noqa: E402

RULES = dict(repetition_penalty=1.1, frequency_penalty=0.2, presence_penalty=0.1, logit_bias={11: -100.0, 12: 2.0, 13: float("-inf")})
SAMPLER = dict(temperature=0.8, top_p=0.9, seed=3)


def build(cfg):
    wts = bench.synth_device_weights(torch, cfg, torch.device("cuda", 0))
    gm = fa.Model(cfg, bench.as_fl_tensors(wts, 0), dtype="bf16")
    del wts
    torch.cuda.empty_cache()
    return gm


def decode(gm, c, first, pos, n, sampled, draws_done):
    if not sampled:
        return gm.decode_greedy(c, first, pos, n)
    return gm.decode_sample(c, first, pos, n, draws_done=draws_done, **SAMPLER)


def kernel_alone(gm, V, T, steps):
    prompt = np.random.RandomState(1234).randint(0, V, size=T).astype(np.uint32)
    c = gm.new_cache(T + steps + 32)
    first = gm.forward_argmax(c, prompt, 0)
    c.set_logit_rules(prompt_ids=prompt, **RULES)
    gm.profile_begin()
    gm.decode_greedy(c, first, T, steps)
    stats = {s["name"]: s for s in gm.profile_end()}
    c.close()
    ru, sel = stats["select_advance[rules]"], stats["select_advance"]
    print("V=%6d  logit_rules %.1f us per launch (%d launches; the full-row ArgMax behind it %.1f us)   bytes moved = V * 16 = %d"
          % (V, ru["total_ms"] / ru["launches"] * 1e3, ru["launches"], sel["total_ms"] / sel["launches"] * 1e3, V * 16))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--prompt", type=int, default=512)
    ap.add_argument("--steps", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=7)
    a = ap.parse_args()
    cfg = MODEL_CONFIGS["mistral-7b"]
    gm = build(cfg)
    T, K = a.prompt, a.steps
    prompt = np.random.RandomState(1234).randint(0, cfg["vocab_size"], size=T).astype(np.uint32)
    prompt[0] = 1
    settings = [("greedy, rules off (fl_decode_greedy)", False, False), ("greedy, rules on", False, True),
                ("sampled, rules off", True, False), ("sampled, rules on", True, True)]
    res = {name: [] for name, _, _ in settings}
    for rep in range(a.rounds):
        for name, sampled, rules in (settings if rep % 2 == 0 else settings[::-1]):
            c = gm.new_cache(T + K + 96)
            first = gm.forward_argmax(c, prompt, 0)
            if rules:
                c.set_logit_rules(prompt_ids=prompt, **RULES)
            t = decode(gm, c, first, T, 16, sampled, 1)          # warm-up + capture
            gm.synchronize()
            t0 = time.perf_counter()
            decode(gm, c, int(t[-1]), T + 16, K, sampled, 17)
            gm.synchronize()
            res[name].append(K / (time.perf_counter() - t0))
            c.close()
    print("mistral-7b (random weights, bf16), prompt %d, %d decode steps, %d rounds interleaved in one process" % (T, K, a.rounds))
    for name, sampled, _ in settings:
        v = np.array(res[name])
        base = np.median(res[settings[2 if sampled else 0][0]])
        print("  %-38s %8.1f tokens/s  (min %.1f .. max %.1f)   %.4f of rules off" % (name, np.median(v), v.min(), v.max(), np.median(v) / base))
    kernel_alone(gm, cfg["vocab_size"], 64, 32)
    gm.close()
    small = dict(cfg, hidden_size=512, intermediate_size=1024, num_hidden_layers=2, num_attention_heads=8, num_key_value_heads=8, vocab_size=152064)
    gs = build(small)
    kernel_alone(gs, small["vocab_size"], 64, 32)
    gs.close()


if __name__ == "__main__":
    main()
