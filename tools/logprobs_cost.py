"""What token log-probabilities cost a decode loop, measured in ONE process on Mistral-7B-shaped random weights.

Four settings interleaved round by round (so drift hits them alike): log-probs off -- fl_decode_greedy, the step every earlier
commit runs and the yardstick here -- and fl_decode_sample_lp (ArgMax) with top_n = 0, 5 and 20.  Every sample is K graph-replayed
steps on a cache of its own behind 16 warm-up steps; reported: median tokens/s with the min .. max spread over the rounds.

Then the kernel alone: its launches inside real decode steps, bracketed by events (fl_profile_*; "select_advance[logprobs]"), at
V = 32 000 (the 7B model above) and V = 152 064 (a two-layer model with that vocabulary: the launch only sees the logits row).
The design bound is two reads of the row from L2, 2 * V * 4 bytes, stated beside each time (the issue allowed three).

    python tools/logprobs_cost.py [--prompt 512] [--steps 256] [--rounds 7]
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


def build(cfg):
    wts = bench.synth_device_weights(torch, cfg, torch.device("cuda", 0))
    gm = fa.Model(cfg, bench.as_fl_tensors(wts, 0), dtype="bf16")
    del wts
    torch.cuda.empty_cache()
    return gm


def decode(gm, c, first, pos, n, top_n):
    if top_n is None:
        return gm.decode_greedy(c, first, pos, n)
    return gm.decode_sample(c, first, pos, n, 0.0, logprobs=top_n)[0]


def kernel_alone(gm, V, T, steps):
    prompt = np.random.RandomState(1234).randint(0, V, size=T).astype(np.uint32)
    for top_n in (0, 5, 20):
        c = gm.new_cache(T + steps + 32)
        first = gm.forward_argmax(c, prompt, 0)
        gm.profile_begin()
        gm.decode_sample(c, first, T, steps, 0.0, logprobs=top_n)
        stats = {s["name"]: s for s in gm.profile_end()}
        c.close()
        lp, sel = stats["select_advance[logprobs]"], stats["select_advance"]
        n = lp["launches"] - 1                                   # (one of them is the launch that writes top_n)
        print("V=%6d top_n=%2d  token_logprobs %.1f us per launch (%d launches; selection launch beside it %.1f us)   row bytes read <= 2 * V * 4 = %d"
              % (V, top_n, lp["total_ms"] / max(n, 1) * 1e3, n, sel["total_ms"] / sel["launches"] * 1e3, 2 * V * 4))


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
    settings = [("log-probs off (fl_decode_greedy)", None), ("top_n = 0", 0), ("top_n = 5", 5), ("top_n = 20", 20)]
    res, toks = {name: [] for name, _ in settings}, {}
    for rep in range(a.rounds):
        for name, top_n in (settings if rep % 2 == 0 else settings[::-1]):
            c = gm.new_cache(T + K + 96)
            first = gm.forward_argmax(c, prompt, 0)
            t = decode(gm, c, first, T, 16, top_n)               # warm-up + capture
            gm.synchronize()
            t0 = time.perf_counter()
            t2 = decode(gm, c, int(t[-1]), T + 16, K, top_n)
            gm.synchronize()
            res[name].append(K / (time.perf_counter() - t0))
            toks[name] = np.concatenate([t, t2])
            c.close()
    base = np.median(res[settings[0][0]])
    print("mistral-7b (random weights, bf16), prompt %d, %d decode steps, %d rounds interleaved in one process" % (T, K, a.rounds))
    for name, _ in settings:
        v = np.array(res[name])
        print("  %-34s %8.1f tokens/s  (min %.1f .. max %.1f)   %.4f of log-probs off   ids equal: %s"
              % (name, np.median(v), v.min(), v.max(), np.median(v) / base, bool(np.array_equal(toks[name], toks[settings[0][0]]))))
    kernel_alone(gm, cfg["vocab_size"], 64, 32)
    gm.close()
    small = dict(cfg, hidden_size=512, intermediate_size=1024, num_hidden_layers=2, num_attention_heads=8, num_key_value_heads=8, vocab_size=152064)
    gs = build(small)
    kernel_alone(gs, small["vocab_size"], 64, 32)
    gs.close()


if __name__ == "__main__":
    main()
