"""What prompt log-probabilities (fl_forward_score / fl_batch_score) cost, measured in ONE process on random weights in bf16.

(a) the score_rows launch alone, between events (fl_op_score_time): V = 32 000 and 152 064, 16 / 256 rows, top_n 0 / 20.
(b) Mistral-7B-shaped: fl_forward_score against fl_forward of the same prompt (the path every earlier commit runs, the yardstick) at
    T = 512 and 4096, top_n 0 and 5, with lm_head blocks (the `score_rows` switch) of 64 / 128 / 256 / 512 rows.
(c) a Qwen2-7B-shaped vocabulary (V = 152 064; a four-layer model of that width: the tail only sees the last hidden rows) at T = 4096.
(d) score_packed of 32 x 64 tokens against 32 single forward_score calls of the same sequences.

(b) - (d): the settings are interleaved round by round (so drift hits them alike), the order reversed every other round; every sample is
a window of whole calls on fresh caches lasting at least 0.25 s, closed by a synchronise; reported: the median ms per call over the
rounds with the min .. max spread.

    python tools/score_cost.py [--rounds 7] [--window 0.25] [--out profiles/r15/score_cost.txt]
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

OUT = {"path": None}


def say(*a):
    """one line to stdout and, as it is measured, to the --out file"""
    line = " ".join(str(x) for x in a)
    print(line, flush=True)
    if OUT["path"]:
        with open(OUT["path"], "a") as f:
            f.write(line + "\n")


def build(cfg, n_layers=None):
    wts = bench.synth_device_weights(torch, cfg, torch.device("cuda", 0), n_layers=n_layers)
    gm = fa.Model(cfg if n_layers is None else dict(cfg, num_hidden_layers=n_layers), bench.as_fl_tensors(wts, 0), dtype="bf16")
    del wts
    torch.cuda.empty_cache()
    return gm


def window(gm, call, seconds):
    """ms per call: whole calls until `seconds` have passed, then a synchronise"""
    gm.synchronize()
    n, t0 = 0, time.perf_counter()
    while True:
        call()
        n += 1
        if time.perf_counter() - t0 >= seconds:
            break
    gm.synchronize()
    return (time.perf_counter() - t0) / n * 1e3


def interleaved(gm, settings, rounds, seconds):
    """settings: [(name, setup, call)]; setup() runs before the window (switches), outside the clock"""
    res = {name: [] for name, _, _ in settings}
    for name, setup, call in settings:                                   # warm every shape once
        setup(); call()
    for rep in range(rounds):
        for name, setup, call in (settings if rep % 2 == 0 else settings[::-1]):
            setup()
            res[name].append(window(gm, call, seconds))
    fa.reload_env()
    return {k: np.array(v) for k, v in res.items()}


def report(res, base):
    b = np.median(res[base])
    for name, v in res.items():
        say("  %-46s %9.3f ms  (min %.3f .. max %.3f)   %.4f x %s" % (name, np.median(v), v.min(), v.max(), np.median(v) / b, base))


def part_a(rounds):
    say("(a) score_rows alone, ms per launch between events (median of %d, min .. max); bytes read = rows * V * 8" % rounds)
    rs = np.random.RandomState(1)
    for V in (32000, 152064):
        for T in (16, 256):
            a = (2.0 * rs.standard_normal((T, V))).astype(np.float32)
            tg = rs.randint(0, V, T).astype(np.uint32)
            for top_n in (0, 20):
                iters = max(8, int(4096 / T))
                v = np.array([fa.op_score_time(a, tg, top_n, iters) for _ in range(rounds)])
                m = np.median(v)
                say("  V=%6d rows=%3d top_n=%2d   %8.4f ms  (min %.4f .. max %.4f)   %6.2f us per row   %.2f TB/s of row reads"
                    % (V, T, top_n, m, v.min(), v.max(), m * 1e3 / T, T * V * 8 / (m * 1e-3) / 1e12))


def forward_settings(gm, V, T, tops, blocks, cap):
    ids = np.random.RandomState(1234).randint(0, V, size=T).astype(np.uint32)
    cache = gm.new_cache(cap)

    def fwd():
        cache.reset(); gm.forward(cache, ids, 0)

    def scored(top_n):
        def f():
            cache.reset(); gm.forward_score(cache, ids, 0, top_n=top_n)
        return f

    settings = [("fl_forward T=%d" % T, fa.reload_env, fwd)]
    for R in blocks:
        for top_n in tops:
            settings.append(("fl_forward_score T=%d top_n=%d score_rows=%d" % (T, top_n, R), (lambda R=R: fa.tune("score_rows", R)), scored(top_n)))
    return settings


def part_b(gm, V, rounds, seconds):
    say("(b) mistral-7b (random weights, bf16): fl_forward_score against fl_forward of the same prompt, fresh cache per call")
    for T in (512, 4096):
        s = forward_settings(gm, V, T, (0, 5), (64, 128, 256, 512), T + 64)
        report(interleaved(gm, s, rounds, seconds), s[0][0])


def part_c(gm, V, rounds, seconds):
    say("(c) qwen2-7b width and vocabulary (V = %d), four layers, T = 4096" % V)
    s = forward_settings(gm, V, 4096, (0, 5), (128, 256, 512), 4096 + 64)
    report(interleaved(gm, s, rounds, seconds), s[0][0])


def part_d(gm, V, rounds, seconds):
    say("(d) mistral-7b: score_packed of 32 x 64 tokens against 32 single forward_score calls, top_n = 0")
    rs = np.random.RandomState(99)
    seqs = [rs.randint(0, V, size=64).astype(np.uint32) for _ in range(32)]
    caches = [gm.new_cache(96) for _ in range(32)]

    def packed():
        for c in caches:
            c.reset()
        gm.score_packed(caches, seqs)

    def singles():
        for c, s in zip(caches, seqs):
            c.reset(); gm.forward_score(c, s, 0)

    s = [("32 single forward_score calls (64 tokens each)", fa.reload_env, singles), ("score_packed, 32 x 64 tokens in one forward", fa.reload_env, packed)]
    report(interleaved(gm, s, rounds, seconds), s[0][0])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--window", type=float, default=0.25)
    ap.add_argument("--out", default=None)
    ap.add_argument("--parts", default="abcd")
    a = ap.parse_args()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").close()
        OUT["path"] = a.out
    say("score_cost: %d rounds, windows of at least %.2f s, one process" % (a.rounds, a.window))
    if "a" in a.parts:
        part_a(a.rounds)
    if "b" in a.parts or "d" in a.parts:
        cfg = MODEL_CONFIGS["mistral-7b"]
        gm = build(cfg)
        if "b" in a.parts:
            part_b(gm, cfg["vocab_size"], a.rounds, a.window)
        if "d" in a.parts:
            part_d(gm, cfg["vocab_size"], a.rounds, a.window)
        gm.close()
    if "c" in a.parts:
        cfg = MODEL_CONFIGS["qwen2-7b"]
        gm = build(cfg, n_layers=4)
        part_c(gm, cfg["vocab_size"], a.rounds, a.window)
        gm.close()


if __name__ == "__main__":
    main()
