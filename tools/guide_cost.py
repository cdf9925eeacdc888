"""What guided decoding (a token-level automaton, fl_cache_set_guide) costs a decode loop, measured in ONE process on
Mistral-7B-shaped random weights in bf16.

Eight settings interleaved round by round (so drift hits them alike), the order reversed every other round: greedy with the guide
off -- fl_decode_greedy, the step every earlier commit runs and the yardstick here -- and with a guide whose every state allows 1 id,
about 1000 ids, or all V ids; and the same four under temperature 0.8 / top-p 0.9 sampling.  Every sample is K graph-replayed steps
on a cache of its own -- so each side captures its graph afresh -- behind 16 warm-up steps; reported: median tokens/s with the
min .. max spread over the rounds.

With a guide on a step has one more launch (guide_mask_kernel: V x 4 bytes written, 8 bytes read per allowed id), and a greedy
step's ArgMax reads the whole masked row instead of the lm_head launch's per-workgroup candidates.  The guides have two states that
lead to each other, so the advance inside the launch finds a real edge at every step.

Then the kernel alone: its launches inside real decode steps, bracketed by events (fl_profile_*; "select_advance[guide]"), at
V = 32 000 (the 7B model above) and V = 152 064 (a two-layer model with that vocabulary: the launch only sees the logits row).

    python tools/guide_cost.py [--prompt 512] [--steps 256] [--rounds 7]
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

SAMPLER = dict(temperature=0.8, top_p=0.9, seed=3)


def build(cfg):
    wts = bench.synth_device_weights(torch, cfg, torch.device("cuda", 0))
    gm = fa.Model(cfg, bench.as_fl_tensors(wts, 0), dtype="bf16")
    del wts
    torch.cuda.empty_cache()
    return gm


def two_state_guide(gm, V, n_allowed):
    """Two states with the same list of n_allowed evenly spread ids, each leading to the other."""
    ids = np.unique(np.linspace(0, V - 1, n_allowed).astype(np.uint32))
    row_ptr = [0, ids.size, 2 * ids.size]
    return fa.Guide(gm, row_ptr, np.concatenate([ids, ids]), np.concatenate([np.ones(ids.size, np.uint32), np.zeros(ids.size, np.uint32)]))


def decode(gm, c, first, pos, n, sampled, draws_done):
    if not sampled:
        return gm.decode_greedy(c, first, pos, n)
    return gm.decode_sample(c, first, pos, n, draws_done=draws_done, **SAMPLER)


def kernel_alone(gm, V, T, steps):
    prompt = np.random.RandomState(1234).randint(0, V, size=T).astype(np.uint32)
    for n_allowed in (1, 1000, V):
        g = two_state_guide(gm, V, n_allowed)
        c = gm.new_cache(T + steps + 32)
        first = gm.forward_argmax(c, prompt, 0)
        c.set_guide(g, 0)
        gm.profile_begin()
        gm.decode_greedy(c, first, T, steps)
        stats = {s["name"]: s for s in gm.profile_end()}
        c.close()
        g.close()
        gu, sel = stats["select_advance[guide]"], stats["select_advance"]
        print("V=%6d  %6d ids allowed  guide_mask %.1f us per launch (%d launches; the full-row ArgMax behind it %.1f us)"
              % (V, n_allowed, gu["total_ms"] / gu["launches"] * 1e3, gu["launches"], sel["total_ms"] / sel["launches"] * 1e3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--prompt", type=int, default=512)
    ap.add_argument("--steps", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=7)
    a = ap.parse_args()
    cfg = MODEL_CONFIGS["mistral-7b"]
    V = cfg["vocab_size"]
    gm = build(cfg)
    T, K = a.prompt, a.steps
    prompt = np.random.RandomState(1234).randint(0, V, size=T).astype(np.uint32)
    prompt[0] = 1
    guides = {0: None, 1: two_state_guide(gm, V, 1), 1000: two_state_guide(gm, V, 1000), V: two_state_guide(gm, V, V)}
    label = {0: "guide off", 1: "guide on, 1 id", 1000: "guide on, ~1000 ids", V: "guide on, all V ids"}
    settings = [("%s, %s" % ("sampled" if sampled else "greedy", label[n]), sampled, n) for sampled in (False, True) for n in (0, 1, 1000, V)]
    res = {name: [] for name, _, _ in settings}
    for rep in range(a.rounds):
        for name, sampled, n in (settings if rep % 2 == 0 else settings[::-1]):
            c = gm.new_cache(T + K + 96)
            first = gm.forward_argmax(c, prompt, 0)
            if guides[n] is not None:
                c.set_guide(guides[n], 0)
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
        base = np.median(res[settings[4 if sampled else 0][0]])
        print("  %-34s %8.1f tokens/s  (min %.1f .. max %.1f)   %.4f of guide off" % (name, np.median(v), v.min(), v.max(), np.median(v) / base))
    for g in guides.values():
        if g is not None:
            g.close()
    kernel_alone(gm, V, 64, 32)
    gm.close()
    small = dict(cfg, hidden_size=512, intermediate_size=1024, num_hidden_layers=2, num_attention_heads=8, num_key_value_heads=8, vocab_size=152064)
    gs = build(small)
    kernel_alone(gs, small["vocab_size"], 64, 32)
    gs.close()


if __name__ == "__main__":
    main()
