"""What the packed forwards of an MXFP4 model gain from streaming the e2m1 nibbles (fl_tune "rows_w4"; from 65 rows
k_gemm_rows128_w4.hip), measured in ONE process on one GPU.  Not a test.

  (a) the projection alone at 65 / 80 / 96 / 128 rows: fl_op_linear_w4_tall on nibbles + scales against fl_op_linear on the bf16 image
      2^e * q, the five Mistral-7B shapes, weights cold (the hooks rotate over copies beyond the Infinity Cache): us per launch,
      achieved TB/s over the weight bytes each reads and TFLOP/s.  These numbers decide rows_wq_plan's rule for 65-128 rows;
  (b) one packed verify step (fl_batch_verify) of n members x r rows on synthetic Mistral-7B MXFP4 behind 512-token prompts, switch 1
      against switch 0 (the parent commit's launches): 4 x 8 and 8 x 8 rows (the 17-64-row kernel, newly routed), 10 x 8 rows (the new kernel where
      the rule serves it) and 12 x 8, 8 x 16 and 16 x 8 rows (beyond the rule: the image);
  (c) fl_batch_prefill of 8 x 16 tokens into empty caches, switch 0 against 1.

The settings alternate inside the process, the order reversed every other round; reported: the median of the rounds with min .. max;
every timed window is at least 0.25 s.  No ratio is promised.

    python tools/packed_w4_ab.py [--rounds 5] [--parts abc] [--out profiles/r25/packed_w4.txt]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402  (first: its HIP runtime must initialise before the product library's, as in bench.py)
import bench  # noqa: E402
import fastllm_amd as fa  # noqa: E402
from fastllm_amd.configs import MODEL_CONFIGS  # noqa: E402
from batch_w4_ab import GRID16  # noqa: E402
from batch_w8_ab import WINDOW, lines, med, say  # noqa: E402


def projections(cfg, rounds):
    h, I, V = cfg["hidden_size"], cfg["intermediate_size"], cfg["vocab_size"]
    d = h // cfg["num_attention_heads"]
    shapes = [("qkv", h + 2 * cfg["num_key_value_heads"] * d, h, 0), ("o_proj", h, h, 0), ("gate/up", 2 * I, h, 1), ("down_proj", h, I, 0), ("lm_head", V, h, 0)]
    say("(a) one projection, us per launch, TB/s over its weight bytes, TFLOP/s: fl_op_linear on the bf16 image | fl_op_linear_w4_tall on e2m1 + e8m0")
    rs = np.random.RandomState(0)
    for name, N, K, epi in shapes:
        q4 = np.resize(rs.randint(0, 256, size=1 << 22).astype(np.uint8), (N, K // 2))
        e4 = np.full((N, K // 32), 127 - 4, dtype=np.uint8)
        t4 = torch.from_numpy(q4).long()
        img = torch.stack([GRID16[t4 & 15], GRID16[t4 >> 4]], dim=2).reshape(N, K).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
        del t4
        for T in (65, 80, 96, 128):
            x = torch.randn(T, K).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
            fn = {"bf16": lambda it: fa.op_linear(x, img, epilogue=epi, iters=it)[1] * 1e3, "w4": lambda it: fa.op_linear_w4_tall(x, q4, e4, epilogue=epi, iters=it)[1] * 1e3}
            iters = {k: max(8, int(WINDOW * 1e6 / f(8)) + 1) for k, f in fn.items()}
            res = {k: [] for k in fn}
            for rep in range(rounds):
                for k in (list(fn) if rep % 2 == 0 else list(fn)[::-1]):
                    res[k].append(fn[k](iters[k]))
            a, c = np.median(res["bf16"]), np.median(res["w4"])
            say("    %-9s %6d x %5d T %3d: bf16 %s us %.2f TB/s %.0f TFLOP/s | w4 %s us %.2f TB/s %.0f TFLOP/s (%d slices) | w4 vs bf16 x%.3f" % (
                name, N, K, T, med(res["bf16"], "%.1f"), 2.0 * N * K / a * 1e-6, 2.0 * T * N * K / a * 1e-6, med(res["w4"], "%.1f"),
                (0.5 + 1.0 / 32) * N * K / c * 1e-6, 2.0 * T * N * K / c * 1e-6, fa.op_linear_w4_tall_plan(T, N, K, epilogue=epi), a / c))


def timed(gm, once):
    """ms per call of once(), over a window of at least WINDOW seconds"""
    once()
    gm.synchronize()
    t0 = time.perf_counter()
    once()
    gm.synchronize()
    reps = max(2, int(WINDOW / (time.perf_counter() - t0)) + 1)
    t0 = time.perf_counter()
    for _ in range(reps):
        once()
    gm.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3


def packed_steps(cfg, T, rounds, parts):
    wts = bench.synth_device_weights(torch, cfg, torch.device("cuda", 0))
    gm = fa.Model(cfg, bench.as_fl_tensors(wts, 0), dtype="bf16", decode_weights="mxfp4")
    del wts
    torch.cuda.empty_cache()
    rs = np.random.RandomState(1234)
    caches, firsts = [], []
    for i in range(16):
        p = rs.randint(0, cfg["vocab_size"], size=T).astype(np.uint32)
        p[0] = 1
        caches.append(gm.new_cache(T + 64))
        firsts.append(gm.forward_argmax(caches[-1], p, 0))
    fresh = [gm.new_cache(64) for _ in range(8)]
    prompts = [rs.randint(0, cfg["vocab_size"], size=16).astype(np.uint32) for _ in range(8)]

    def verify(n, r):
        drafts = [rs.randint(0, cfg["vocab_size"], size=r - 1).astype(np.uint32) for _ in range(n)]

        def once():
            for c in caches[:n]:
                c.truncate(T)
            gm.verify_packed(caches[:n], firsts[:n], drafts, [T] * n)
        return once

    def prefill():
        for c in fresh:
            c.truncate(0)
        gm.prefill_packed(fresh, prompts)

    jobs = []
    if "b" in parts:
        jobs += [("(b) packed verify %2d x %2d rows" % (n, r), verify(n, r)) for n, r in ((4, 8), (8, 8), (10, 8), (12, 8), (8, 16), (16, 8))]
    if "c" in parts:
        jobs += [("(c) packed prefill 8 x 16 tokens", prefill)]
    say("(b, c) one packed forward on Mistral-7B MXFP4 (random weights; verify behind %d-token prompts), ms per call:" % T)
    try:
        for what, once in jobs:
            res = {0: [], 1: []}
            for rep in range(rounds):
                for sw in ((0, 1) if rep % 2 == 0 else (1, 0)):
                    fa.tune("rows_w4", sw)
                    res[sw].append(timed(gm, once))
            say("    %s: switch 0 (bf16 image, the parent's launches) %s | switch 1 (nibbles) %s | x%.3f" % (
                what, med(res[0]), med(res[1]), np.median(res[0]) / np.median(res[1])))
    finally:
        fa.tune("rows_w4", 0)
    for c in caches + fresh:
        c.close()
    gm.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--prompt", type=int, default=512)
    ap.add_argument("--parts", default="abc", help="which of (a), (b), (c) to run")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.rounds >= 5
    cfg = MODEL_CONFIGS["mistral-7b"]
    say("packed forwards of 2-128 rows of an MXFP4 model on e2m1 nibbles: one GPU, %d rounds per setting, settings interleaved in one process, median (min .. max)" % a.rounds)
    if "a" in a.parts:
        projections(cfg, a.rounds)
    if "b" in a.parts or "c" in a.parts:
        packed_steps(cfg, a.prompt, a.rounds, a.parts)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
