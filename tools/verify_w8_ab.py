"""What the verify step of an FP8 model gains from streaming the e4m3 bytes (k_gemm_rows_w8.hip, fl_tune "verify_w8"), measured in ONE
process on one GPU.  Not a test.

  (a) the projection alone: fl_op_linear_w8 on q / s against fl_op_linear on the bf16 image s * q, the five Mistral-7B shapes at
      T = 2 / 8 / 16 rows, weights cold (both hooks rotate over copies beyond the Infinity Cache): us per launch and achieved TB/s
      over the weight bytes each reads;
  (b) one verify step of 4 / 8 / 16 rows on synthetic Mistral-7B FP8 behind a 512-token prompt, switch 1 against switch 0 (the
      parent commit's launches), next to the graph-replayed FP8 decode step it stands for;
  (c) fl_decode_lookup with a corpus that holds the loop's own output (iterated towards a fixed point: forced acceptance where the
      weights allow one -- random weights' near-tied logits may not; the lines report what was accepted) under both switch values
      against fl_decode_greedy, tokens/s.

The switch alternates inside the process, the order reversed every other round; reported: the median of the rounds with min .. max;
every timed window is at least 0.25 s.  No ratio is promised; acceptance on real text cannot be measured with random weights.

    python tools/verify_w8_ab.py [--rounds 5] [--parts abc] [--out profiles/r20/verify_w8.txt]
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

WINDOW = 0.27                                          # seconds per timed window (the floor asked for is 0.25)
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def med(xs, fmt="%.3f"):
    return (fmt + " (" + fmt + " .. " + fmt + ")") % (np.median(xs), min(xs), max(xs))


def projections(cfg, rounds):
    h, I, V = cfg["hidden_size"], cfg["intermediate_size"], cfg["vocab_size"]
    d = h // cfg["num_attention_heads"]
    shapes = [("qkv", h + 2 * cfg["num_key_value_heads"] * d, h, 0), ("o_proj", h, h, 0), ("gate/up", 2 * I, h, 1), ("down_proj", h, I, 0), ("lm_head", V, h, 0)]
    say("(a) one projection, us per launch and TB/s over its weight bytes: fl_op_linear on the bf16 image | fl_op_linear_w8 on e4m3")
    rs = np.random.RandomState(0)
    for name, N, K, epi in shapes:
        q = np.resize(rs.randint(0, 0x78, size=1 << 22).astype(np.uint8), (N, K))     # finite codes, values below 1
        s = np.full(N, 2.0 ** -4, dtype=np.float32)
        img = (torch.from_numpy(q).view(torch.float8_e4m3fn).to(torch.bfloat16) * 2.0 ** -4).view(torch.int16).numpy().view(np.uint16)
        for T in (2, 8, 16):
            x = torch.randn(T, K).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
            fn = {"bf16": lambda it: fa.op_linear(x, img, epilogue=epi, iters=it)[1] * 1e3, "fp8": lambda it: fa.op_linear_w8(x, q, s, epilogue=epi, iters=it)[1] * 1e3}
            iters = {k: max(8, int(WINDOW * 1e6 / f(8)) + 1) for k, f in fn.items()}
            res = {k: [] for k in fn}
            for rep in range(rounds):
                for k in (("bf16", "fp8") if rep % 2 == 0 else ("fp8", "bf16")):
                    res[k].append(fn[k](iters[k]))
            a, b = np.median(res["bf16"]), np.median(res["fp8"])
            say("    %-9s %6d x %5d T %2d: bf16 %s us %.2f TB/s | fp8 %s us %.2f TB/s (%d slices) | x%.3f" % (
                name, N, K, T, med(res["bf16"], "%.1f"), 2.0 * N * K / a * 1e-6, med(res["fp8"], "%.1f"), 1.0 * N * K / b * 1e-6,
                fa.op_linear_w8_plan(T, N, K, epilogue=epi), a / b))


def timed(fn, rounds, settings, sync):
    """fn(setting) once per call -> ms per call for every setting: windows of WINDOW seconds, settings alternating"""
    reps = {}
    for s in settings:
        fn(s); sync()
        t0 = time.perf_counter()
        for _ in range(4):
            fn(s)
        sync()
        reps[s] = max(4, int(WINDOW / ((time.perf_counter() - t0) / 4)) + 1)
    res = {s: [] for s in settings}
    for rep in range(rounds):
        for s in (settings if rep % 2 == 0 else settings[::-1]):
            sync()
            t0 = time.perf_counter()
            for _ in range(reps[s]):
                fn(s)
            sync()
            res[s].append((time.perf_counter() - t0) / reps[s] * 1e3)
    return res


def model_level(cfg, T, rounds, parts):
    wts = bench.synth_device_weights(torch, cfg, torch.device("cuda", 0))
    gm = fa.Model(cfg, bench.as_fl_tensors(wts, 0), dtype="bf16", decode_weights="e4m3")
    del wts
    torch.cuda.empty_cache()
    V = cfg["vocab_size"]
    prompt = np.random.RandomState(1234).randint(0, V, size=T).astype(np.uint32)
    prompt[0] = 1
    K = 768
    c = gm.new_cache(T + K + 96)
    first = gm.forward_argmax(c, prompt, 0)
    want = gm.decode_greedy(c, first, T, K)
    c.truncate(T)
    # (b)
    say("(b) one verify step behind a %d-token prompt on Mistral-7B FP8 (random weights), ms per call (forward + selection + copy-back + sync):" % T)
    for rows in (4, 8, 16) if "b" in parts else ():
        def step(sw):
            fa.tune("verify_w8", sw)
            c.truncate(T)
            gm.forward_verify(c, first, want[:rows - 1], T)
        res = timed(step, rounds, [0, 1], gm.synchronize)
        say("    %2d rows: switch 0 (bf16 image, the parent's launches) %s | switch 1 (e4m3) %s | x%.3f" % (
            rows, med(res[0]), med(res[1]), np.median(res[0]) / np.median(res[1])))

    def greedy(_):
        c.truncate(T)
        gm.decode_greedy(c, first, T, 256)
    greedy(0)
    res = timed(greedy, rounds, [0], gm.synchronize)
    say("    the FP8 decode step (fl_decode_greedy, graph replay, 256 steps per call): %s ms per step" % med([x / 256 for x in res[0]], "%.4f"))
    # (c)
    # the corpus holds what the loop itself emits under each switch value: with random weights (near-tied logits) the verify rows do not
    # always pick the decode kernel's id, so the greedy continuation is iterated to the loop's own fixed point (at most 6 passes)
    say("(c) fl_decode_lookup, its own output as the corpus, %d tokens, tokens/s:" % K)
    stats, corpus = {}, {}
    for sw in (0, 1):
        fa.tune("verify_w8", sw)
        cur = want
        for _ in range(6):
            c.truncate(T)
            got = gm.decode_lookup(c, np.concatenate([prompt, [first], cur]).astype(np.uint32), first, T, K, max_draft=15)
            if np.array_equal(got, cur):
                break
            cur = got
        corpus[sw] = np.concatenate([prompt, [first], cur]).astype(np.uint32)
    for md in (7, 15):
        def loop(sw):
            c.truncate(T)
            if sw < 0:
                gm.decode_greedy(c, first, T, K)
                return
            fa.tune("verify_w8", sw)
            got, stats[md, sw] = gm.decode_lookup(c, corpus[sw], first, T, K, max_draft=md, return_stats=True)
            stats[md, sw]["equal"] = bool(np.array_equal(got, corpus[sw][T + 1:]))
        res = timed(loop, rounds, [-1, 0, 1], gm.synchronize)
        tps = {s: [K / (x * 1e-3) for x in res[s]] for s in res}
        say("    max_draft %2d: fl_decode_greedy %s | switch 0 %s | switch 1 %s | switch 1 / switch 0 x%.3f, switch 1 / greedy x%.3f" % (
            md, med(tps[-1], "%.1f"), med(tps[0], "%.1f"), med(tps[1], "%.1f"), np.median(tps[1]) / np.median(tps[0]), np.median(tps[1]) / np.median(tps[-1])))
        for sw in (0, 1):
            s = stats[md, sw]
            say("        switch %d: %d steps, %d drafted, %d accepted; ids equal the corpus: %s" % (sw, s["steps"], s["drafted"], s["accepted"], s["equal"]))
    fa.tune("verify_w8", 1)
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
    say("verify step of an FP8 model on e4m3 bytes: one GPU, %d rounds per setting, settings interleaved in one process, median (min .. max)" % a.rounds)
    if "a" in a.parts:
        projections(cfg, a.rounds)
    model_level(cfg, a.prompt, a.rounds, a.parts)
    say("acceptance on real text was not and cannot be measured with random weights; no ratio is promised")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
