"""What a decode batch of 17-64 streams of an MXFP4 model gains from streaming the e2m1 nibbles (k_gemm_rows64_w4.hip, fl_tune
"rows_w4"), measured in ONE process on one GPU.  Not a test.

  (a) the projection alone at 17 / 32 / 64 rows: fl_op_linear_w4_wide on nibbles + scales against fl_op_linear on the bf16 image
      2^e * q and against fl_op_linear_w8_wide on e4m3 bytes, the five Mistral-7B shapes, weights cold (the hooks rotate over copies
      beyond the Infinity Cache): us per launch and achieved TB/s over the weight bytes each reads;
  (b) the decode step of a batch of 17 / 32 / 64 streams on synthetic Mistral-7B MXFP4 behind 512-token prompts, switch 1 against
      switch 0 (the parent commit's launches): ms per step of a 64-step fl_batch_decode (graph replay), a fresh Batch per sample (the
      switch is read when a Batch is created).

The settings alternate inside the process, the order reversed every other round; reported: the median of the rounds with min .. max;
every timed window is at least 0.25 s.  No ratio is promised.

    python tools/batch_w4_ab.py [--rounds 5] [--parts ab] [--out profiles/r24/batch_w4.txt]
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
from batch_w8_ab import STEPS, WINDOW, lines, med, say  # noqa: E402

GRID = torch.tensor([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0])
GRID16 = torch.cat([GRID, -GRID]) * 2.0 ** -4


def projections(cfg, rounds):
    h, I, V = cfg["hidden_size"], cfg["intermediate_size"], cfg["vocab_size"]
    d = h // cfg["num_attention_heads"]
    shapes = [("qkv", h + 2 * cfg["num_key_value_heads"] * d, h, 0), ("o_proj", h, h, 0), ("gate/up", 2 * I, h, 1), ("down_proj", h, I, 0), ("lm_head", V, h, 0)]
    say("(a) one projection, us per launch and TB/s over its weight bytes: fl_op_linear on the bf16 image | fl_op_linear_w8_wide on e4m3 | fl_op_linear_w4_wide on e2m1 + e8m0")
    rs = np.random.RandomState(0)
    for name, N, K, epi in shapes:
        q4 = np.resize(rs.randint(0, 256, size=1 << 22).astype(np.uint8), (N, K // 2))
        e4 = np.full((N, K // 32), 127 - 4, dtype=np.uint8)
        t4 = torch.from_numpy(q4).long()
        img = torch.stack([GRID16[t4 & 15], GRID16[t4 >> 4]], dim=2).reshape(N, K).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
        del t4
        q8 = np.resize(rs.randint(0, 0x78, size=1 << 22).astype(np.uint8), (N, K))
        s8 = np.full(N, 2.0 ** -4, dtype=np.float32)
        for T in (17, 32, 64):
            x = torch.randn(T, K).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
            fn = {"bf16": lambda it: fa.op_linear(x, img, epilogue=epi, iters=it)[1] * 1e3, "fp8": lambda it: fa.op_linear_w8_wide(x, q8, s8, epilogue=epi, iters=it)[1] * 1e3,
                  "w4": lambda it: fa.op_linear_w4_wide(x, q4, e4, epilogue=epi, iters=it)[1] * 1e3}
            iters = {k: max(8, int(WINDOW * 1e6 / f(8)) + 1) for k, f in fn.items()}
            res = {k: [] for k in fn}
            for rep in range(rounds):
                for k in (list(fn) if rep % 2 == 0 else list(fn)[::-1]):
                    res[k].append(fn[k](iters[k]))
            a, b, c = (np.median(res[k]) for k in ("bf16", "fp8", "w4"))
            say("    %-9s %6d x %5d T %2d: bf16 %s us %.2f TB/s | fp8 %s us %.2f TB/s (%d slices) | w4 %s us %.2f TB/s (%d slices) | w4 vs bf16 x%.3f, vs fp8 x%.3f" % (
                name, N, K, T, med(res["bf16"], "%.1f"), 2.0 * N * K / a * 1e-6, med(res["fp8"], "%.1f"), 1.0 * N * K / b * 1e-6,
                fa.op_linear_w8_wide_plan(T, N, K, epilogue=epi), med(res["w4"], "%.1f"), (0.5 + 1.0 / 32) * N * K / c * 1e-6,
                fa.op_linear_w4_wide_plan(T, N, K, epilogue=epi), a / c, b / c))


def batch_steps(cfg, T, rounds):
    wts = bench.synth_device_weights(torch, cfg, torch.device("cuda", 0))
    gm = fa.Model(cfg, bench.as_fl_tensors(wts, 0), dtype="bf16", decode_weights="mxfp4")
    del wts
    torch.cuda.empty_cache()
    rs = np.random.RandomState(1234)
    caches, firsts = [], []
    for i in range(64):
        p = rs.randint(0, cfg["vocab_size"], size=T).astype(np.uint32)
        p[0] = 1
        caches.append(gm.new_cache(T + 2 * STEPS + 16))
        firsts.append(gm.forward_argmax(caches[-1], p, 0))
    say("(b) one decode step of a batch behind %d-token prompts on Mistral-7B MXFP4 (random weights), ms per step of a %d-step fl_batch_decode:" % (T, STEPS))
    try:
        for B in (17, 32, 64):
            res = {0: [], 1: []}
            for rep in range(rounds):
                for sw in ((0, 1) if rep % 2 == 0 else (1, 0)):
                    fa.tune("rows_w4", sw)
                    for c in caches[:B]:
                        c.truncate(T)
                    b = fa.Batch(gm, caches[:B])
                    b.decode(firsts[:B], [T] * B, 4)                            # (captures the step's graph)
                    gm.synchronize()
                    t0 = time.perf_counter()
                    b.decode(firsts[:B], [T + 4] * B, STEPS)
                    gm.synchronize()
                    res[sw].append((time.perf_counter() - t0) / STEPS * 1e3)
                    b.close()
            say("    B %2d: switch 0 (bf16 image, the parent's launches) %s | switch 1 (nibbles) %s | x%.3f | %.0f -> %.0f tokens/s" % (
                B, med(res[0]), med(res[1]), np.median(res[0]) / np.median(res[1]), B / np.median(res[0]) * 1e3, B / np.median(res[1]) * 1e3))
    finally:
        fa.tune("rows_w4", 0)
    for c in caches:
        c.close()
    gm.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--prompt", type=int, default=512)
    ap.add_argument("--parts", default="ab", help="which of (a), (b) to run")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.rounds >= 5
    cfg = MODEL_CONFIGS["mistral-7b"]
    say("decode batches of 17-64 streams of an MXFP4 model on e2m1 nibbles: one GPU, %d rounds per setting, settings interleaved in one process, median (min .. max)" % a.rounds)
    if "a" in a.parts:
        projections(cfg, a.rounds)
    if "b" in a.parts:
        batch_steps(cfg, a.prompt, a.rounds)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
