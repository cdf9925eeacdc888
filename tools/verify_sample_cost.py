"""What the sampled verify step (fl_forward_verify_ex, verify_sample_kernel) costs, measured in ONE process on one GPU.  Not a test.

  (a) the verify_sample launch alone, between two events (fl_op_verify_sample_time), for T = 1, 8, 16 rows at V = 32 000 and
      V = 152 064 with three samplers -- Sampling::All, top-p 0.9, top-k 40 -- and beside it T one-row select_advance launches of the
      same rows (what the plain loop spends on selecting the same T tokens);
  (b) one verify step of 8 rows on synthetic Mistral-7B bf16 behind a 512-token prompt: sampled against greedy (the parent commit's
      verify path: verify_select) on the same cache state;
  (c) fl_decode_lookup_ex at FORCED acceptance against fl_decode_sample_ex, 256 tokens each: top_k = 1 and a corpus that holds the
      continuation -- the only way to force acceptance with random weights.  The continuation is the loop's own (found by feeding
      it its output until it reproduces it): in bf16 the rows of a verify step and the one-row steps of the plain loop part at
      near-ties of the two largest logits, which random weights are full of.

All settings alternate inside the process, the order reversed every other round; reported: the median of the rounds with min .. max;
every timed window is at least 0.25 s.  Acceptance on real text cannot be measured with random weights: (c) is the speed when every
draft is right, never a typical speed-up.

    python tools/verify_sample_cost.py [--rounds 7] [--out profiles/r14/verify_sample_cost.txt]
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
SAMPLERS = [("Sampling::All t=1.0", dict(temperature=1.0)), ("top-p 0.9 t=0.8", dict(temperature=0.8, top_p=0.9)),
            ("top-k 40 t=0.8", dict(temperature=0.8, top_k=40))]
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def med(xs, fmt="%.3f"):
    return (fmt + " (" + fmt + " .. " + fmt + ")") % (np.median(xs), min(xs), max(xs))


def launch_alone(rounds):
    for V in (32000, 152064):
        rows = (np.random.RandomState(V).randn(16, V) * 2.5).astype(np.float32)
        settings = [(T, name, sp) for T in (1, 8, 16) for name, sp in SAMPLERS]
        iters, res = {}, {}
        for T, name, sp in settings:                    # calibrate: as many repetitions as fill the window
            a, b = fa.op_verify_sample_time(rows[:T], sp["temperature"], (8, 8), top_p=sp.get("top_p"), top_k=sp.get("top_k"))
            iters[T, name] = (max(8, int(WINDOW * 1e3 / a) + 1), max(8, int(WINDOW * 1e3 / b) + 1))
            res[T, name] = ([], [])
        for rep in range(rounds):
            for T, name, sp in (settings if rep % 2 == 0 else settings[::-1]):
                a, b = fa.op_verify_sample_time(rows[:T], sp["temperature"], iters[T, name], top_p=sp.get("top_p"), top_k=sp.get("top_k"))
                res[T, name][0].append(a * 1e3)
                res[T, name][1].append(b * 1e3)
        say("(a) V = %d: us per verify_sample launch of T rows | us per T one-row select_advance launches | ratio of the medians" % V)
        for T, name, _ in settings:
            a, b = res[T, name]
            say("    T %2d  %-20s %s | %s | %.3f" % (T, name, med(a, "%.1f"), med(b, "%.1f"), np.median(a) / np.median(b)))


def build(cfg):
    wts = bench.synth_device_weights(torch, cfg, torch.device("cuda", 0))
    gm = fa.Model(cfg, bench.as_fl_tensors(wts, 0), dtype="bf16")
    del wts
    torch.cuda.empty_cache()
    return gm


def verify_step(gm, prompt, T, rounds):
    c = gm.new_cache(T + 64)
    first = gm.forward_argmax(c, prompt, 0)
    draft = gm.decode_greedy(c, first, T, 7)            # 8 rows: the token and 7 drafts
    c.truncate(T)
    forms = [("greedy (verify_select)", None)] + [("sampled, " + name, sp) for name, sp in SAMPLERS]

    def step(sp):
        if sp is None:
            gm.forward_verify(c, first, draft, T)
        else:
            gm.forward_verify(c, first, draft, T, seed=3, draws_done=1, **sp)
        c.truncate(T)                                   # host state only: the same cache state for every call

    reps = {}
    for name, sp in forms:
        step(sp)
        gm.synchronize()
        t0 = time.perf_counter()
        for _ in range(8):
            step(sp)
        reps[name] = max(8, int(WINDOW / ((time.perf_counter() - t0) / 8)) + 1)
    res = {name: [] for name, _ in forms}
    for rep in range(rounds):
        for name, sp in (forms if rep % 2 == 0 else forms[::-1]):
            gm.synchronize()
            t0 = time.perf_counter()
            for _ in range(reps[name]):
                step(sp)
            res[name].append((time.perf_counter() - t0) / reps[name] * 1e3)
    say("(b) one verify step of 8 rows behind a %d-token prompt, ms per call (forward + selection + copy-back + sync):" % T)
    g = np.median(res[forms[0][0]])
    for name, _ in forms:
        say("    %-32s %s   x%.4f of greedy" % (name, med(res[name]), np.median(res[name]) / g))
    c.close()


def loop(gm, prompt, T, K, rounds):
    sp = dict(temperature=0.8, top_k=1, seed=3)
    c = gm.new_cache(T + K + 96)
    first = gm.forward_sample(c, prompt, 0, draws_done=0, **sp)
    plain = gm.decode_sample(c, first, T, K, draws_done=1, **sp)
    forms = [("fl_decode_sample_ex", 0), ("fl_decode_lookup_ex max_draft 7", 7), ("fl_decode_lookup_ex max_draft 15", 15)]

    def lookup(cont, md, n):
        c.truncate(T)
        return gm.decode_lookup(c, np.concatenate([prompt, [first], cont]).astype(np.uint32), first, T, n, max_draft=md, return_stats=True,
                                draws_done=1, **sp)

    # The corpus must hold the continuation THE LOOP ITSELF produces: with random weights the bf16 logits of a multi-row call and of a
    # one-row call disagree on near-ties of the top two, so the plain loop's tokens are not the verify rows' tokens for long.  Feed the
    # loop its own output until it reproduces it (every pass confirms at least one more step).
    cont, note = {}, {}
    for name, md in forms[1:]:
        cur, passes = plain, 0
        for passes in range(1, 33):
            got, _ = lookup(cur, md, K)
            if np.array_equal(got, cur):
                break
            cur = got
        cont[name] = cur
        k = int(np.argmax(cur != plain)) if not np.array_equal(cur, plain) else K
        gap = ""
        if k < K:                                       # the one-row logits where the two loops part: how close the top two are
            c.truncate(T)
            lg = None
            for i, t in enumerate([first] + plain[:k].tolist()):
                lg = gm.forward(c, [t], T + i)
            top2 = np.sort(lg)[-2:]
            gap = ", top-two gap there %.3g of max |logit| %.3g" % (top2[1] - top2[0], np.abs(lg).max())
        note[name] = "fixed point after %d pass(es): %s; first id that differs from the plain loop's: %s%s" % (
            passes, bool(np.array_equal(lookup(cur, md, K)[0], cur)), k if k < K else "none", gap)

    def run(name, md, n):
        if md == 0:
            c.truncate(T)
            return gm.decode_sample(c, first, T, n, draws_done=1, **sp), None
        return lookup(cont[name], md, n)

    res, stats = {f: [] for f, _ in forms}, {}
    for name, md in forms:
        run(name, md, 32)                               # warm-up (graph capture, scratch)
    for rep in range(rounds):
        for name, md in (forms if rep % 2 == 0 else forms[::-1]):
            gm.synchronize()
            t0 = time.perf_counter()
            _, st = run(name, md, K)
            gm.synchronize()
            dt = time.perf_counter() - t0
            n = 1
            while dt < WINDOW:                          # a window of at least 0.25 s: repeat the request
                _, st = run(name, md, K)
                gm.synchronize()
                dt, n = time.perf_counter() - t0, n + 1
            res[name].append(n * K / dt)
            stats[name] = st
    say("(c) %d tokens behind a %d-token prompt, top_k = 1, the corpus holds the loop's own continuation (FORCED acceptance), tokens/s:" % (K, T))
    g = np.median(res[forms[0][0]])
    for name, _ in forms:
        extra = ""
        if stats[name] is not None:
            s = stats[name]
            extra = "; %d steps, %d drafted, %d accepted" % (s["steps"], s["drafted"], s["accepted"])
        say("    %-34s %s   x%.3f of the plain sampled loop%s" % (name, med(res[name], "%.1f"), np.median(res[name]) / g, extra))
    for name, _ in forms[1:]:
        say("    %s: %s" % (name, note[name]))
    c.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--prompt", type=int, default=512)
    ap.add_argument("--steps", type=int, default=256)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.rounds >= 7
    say("sampled verify step: cost on one GPU, %d rounds per setting, settings interleaved in one process, median (min .. max)" % a.rounds)
    launch_alone(a.rounds)
    cfg = MODEL_CONFIGS["mistral-7b"]
    gm = build(cfg)
    prompt = np.random.RandomState(1234).randint(0, cfg["vocab_size"], size=a.prompt).astype(np.uint32)
    prompt[0] = 1
    say("mistral-7b (random weights, bf16), V = %d" % cfg["vocab_size"])
    verify_step(gm, prompt, a.prompt, a.rounds)
    loop(gm, prompt, a.prompt, a.steps, a.rounds)
    say("acceptance on real text was not and cannot be measured with random weights: (c) is the speed when every draft is right")
    gm.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
