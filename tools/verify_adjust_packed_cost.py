"""What logit rules, a guide and log-probs cost inside a PACKED verify step (fl_batch_verify_lp, verify_adjust_packed_kernel), measured
in ONE process on one GPU.  Not a test.

  (a) the verify_adjust_packed launch alone, between two events (fl_op_verify_adjust_packed with iters), for packs of 8 x 8 and 32 x 8
      rows at V = 32 000 and V = 152 064 in its three forms: rules only, a guide whose states allow ~1000 ids only, both;
  (b) one packed step of 32 members x 8 rows on synthetic Mistral-7B bf16 behind 512-token prompts: every member ruled + guided with
      top_n 5 log-probs (fl_batch_verify_lp) against the same pack of bare caches through fl_batch_verify (the parent commit's path,
      which this commit runs unchanged for such a pack);
  (c) with --parent DIR (a built checkout of the parent commit): bench.py --gpus 1 --steps 256 --warmup 8 there and here, alternating,
      three runs each, with the token checksum.  Without it: not recorded.

All settings alternate inside the process, the order reversed every other round; reported: the median of the rounds with min .. max;
every timed window is at least 0.25 s.  No ratio is promised; acceptance on real text cannot be measured with random weights.

    python tools/verify_adjust_packed_cost.py [--rounds 5] [--parent DIR] [--out profiles/r19/verify_adjust_packed_cost.txt]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402  (first: its HIP runtime must initialise before the product library's, as in bench.py)
import bench  # noqa: E402
import fastllm_amd as fa  # noqa: E402
from fastllm_amd.configs import MODEL_CONFIGS  # noqa: E402
sys.path.insert(0, os.path.join(ROOT, "tools"))
from verify_adjust_cost import ALLOWED, RULES, WINDOW, automaton, med  # noqa: E402

ROWS = 8                                               # rows per member
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def launch_alone(rounds):
    for V in (32000, 152064):
        rs = np.random.RandomState(V)
        scal = (RULES["repetition_penalty"], RULES["frequency_penalty"], RULES["presence_penalty"])
        row_ptr, tokens, nxt, _ = automaton(V)
        packs = {}
        for n in (8, 32):
            T = n * ROWS
            biases = np.zeros((n, V), np.float32)
            biases[:, rs.choice(V, 64, replace=False)] = 1.0
            packs[n] = dict(logits=(rs.randn(T, V) * 2.5).astype(np.float32), offsets=np.arange(n + 1) * ROWS, ids=rs.randint(0, V, T).astype(np.uint32),
                            rules=dict(words=rs.randint(0, 4, (n, V)).astype(np.uint32), biases=biases, scalars=np.tile(scal, (n, 1))),
                            guide=dict(guide=(row_ptr, tokens, nxt), states=(np.arange(T) % 4).astype(np.uint32)))
        forms = {"rules only": ("rules",), "guide only (~%d ids)" % ALLOWED: ("guide",), "rules + guide": ("rules", "guide")}
        settings = [(n, name) for n in (8, 32) for name in forms]

        def run(n, name, iters):
            p, kw = packs[n], {}
            for part in forms[name]:
                kw.update(p[part])
            return fa.op_verify_adjust_packed(p["logits"], p["offsets"], p["ids"], iters=iters, **kw) * 1e3

        iters = {s: max(8, int(WINDOW * 1e6 / run(s[0], s[1], 8)) + 1) for s in settings}
        res = {s: [] for s in settings}
        for rep in range(rounds):
            for s in (settings if rep % 2 == 0 else settings[::-1]):
                res[s].append(run(s[0], s[1], iters[s]))
        say("(a) V = %d: us per verify_adjust_packed launch on one block of n members x %d rows" % (V, ROWS))
        for n, name in settings:
            say("    %2d x %d  %-24s %s" % (n, ROWS, name, med(res[n, name], "%.1f")))


def packed_step(gm, cfg, T, rounds, n=32):
    V = cfg["vocab_size"]
    row_ptr, tokens, nxt, _ = automaton(V)
    guide = fa.Guide(gm, row_ptr, tokens, nxt)
    rs = np.random.RandomState(1234)
    prompts = rs.randint(0, V, size=(n, T)).astype(np.uint32)
    prompts[:, 0] = 1
    bias = {int(j): 1.0 for j in np.random.RandomState(7).choice(V, 64, replace=False)}
    bare = [gm.new_cache(T + 64) for _ in range(n)]
    full = [gm.new_cache(T + 64) for _ in range(n)]
    firsts = [gm.forward_argmax(c, p, 0) for c, p in zip(bare, prompts)]
    assert [gm.forward_argmax(c, p, 0) for c, p in zip(full, prompts)] == firsts

    def install():
        for c, p in zip(full, prompts):
            c.set_logit_rules(prompt_ids=p, logit_bias=bias, **RULES)
            c.set_guide(guide, 0)

    install()
    # drafts the guide can reach: each member's own ruled, guided continuation
    drafts = [gm.decode_sample(c, f, T, ROWS - 1, 0.0, logprobs=5)[0] for c, f in zip(full, firsts)]
    drafts_bare = [gm.decode_greedy(c, f, T, ROWS - 1) for c, f in zip(bare, firsts)]
    forms = ["bare caches, fl_batch_verify (the parent's path)", "rules + guide + top_n 5, fl_batch_verify_lp"]

    def step(name):
        if name == forms[0]:
            for c in bare:
                c.truncate(T)
            gm.verify_packed(bare, firsts, drafts_bare, [T] * n)
            return
        for c in full:
            c.truncate(T)
        install()                                       # the tables and states as before the step (part of the window; timed alone below)
        gm.verify_packed_lp(full, firsts, drafts, [T] * n, logprobs=[5] * n)

    def install_only():
        for c in full:
            c.truncate(T)
        install()
        gm.synchronize()

    timed = forms + ["(the re-install of %d members alone, inside the ruled window)" % n]
    fn = {name: (lambda k=name: step(k)) for name in forms}
    fn[timed[-1]] = install_only
    reps = {}
    for name in timed:
        fn[name]()
        gm.synchronize()
        t0 = time.perf_counter()
        for _ in range(4):
            fn[name]()
        gm.synchronize()
        reps[name] = max(4, int(WINDOW / ((time.perf_counter() - t0) / 4)) + 1)
    res = {name: [] for name in timed}
    for rep in range(rounds):
        for name in (timed if rep % 2 == 0 else timed[::-1]):
            gm.synchronize()
            t0 = time.perf_counter()
            for _ in range(reps[name]):
                fn[name]()
            gm.synchronize()
            res[name].append((time.perf_counter() - t0) / reps[name] * 1e3)
    say("(b) one packed step of %d members x %d rows behind %d-token prompts, ms per call (forward + adjust + selection + scoring + count + copy-back + sync):" % (n, ROWS, T))
    g = np.median(res[forms[0]])
    for name in timed:
        say("    %-62s %s   x%.4f of the bare step" % (name, med(res[name]), np.median(res[name]) / g))
    for c in bare + full:
        c.close()
    guide.close()


def bench_ab(parent):
    say("(c) bench.py --gpus 1 --steps 256 --warmup 8, parent and this commit alternating, three runs each:")
    if not parent:
        say("    not recorded (no --parent checkout given)")
        return
    for run in range(3):
        for who, cwd in (("parent", parent), ("this", ROOT)):
            env = dict(os.environ)
            env.pop("FL_LIB_PATH", None)
            out = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "256", "--warmup", "8"], cwd=cwd, env=env, capture_output=True,
                                 text=True, timeout=600)
            rec = next((json.loads(ln) for ln in reversed(out.stdout.splitlines()) if ln.startswith("{")), None)
            if out.returncode != 0 or rec is None:
                say("    run %d  %-6s  not recorded (bench.py exited with %d)" % (run + 1, who, out.returncode))
                continue
            say("    run %d  %-6s  %.2f tokens/s   %.4f ms/step   tokens_crc32 %d" % (run + 1, who, rec["value"], rec["ms_per_step"], rec["tokens_crc32"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--prompt", type=int, default=512)
    ap.add_argument("--parent", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.rounds >= 5
    say("packed verify step with rules, guide and log-probs: cost on one GPU, %d rounds per setting, settings interleaved in one process, median (min .. max)" % a.rounds)
    launch_alone(a.rounds)
    cfg = MODEL_CONFIGS["mistral-7b"]
    wts = bench.synth_device_weights(torch, cfg, torch.device("cuda", 0))
    gm = fa.Model(cfg, bench.as_fl_tensors(wts, 0), dtype="bf16")
    del wts
    torch.cuda.empty_cache()
    say("mistral-7b (random weights, bf16), V = %d" % cfg["vocab_size"])
    packed_step(gm, cfg, a.prompt, a.rounds)
    gm.close()
    del gm
    torch.cuda.empty_cache()
    bench_ab(a.parent)
    say("acceptance on real text was not and cannot be measured with random weights; no ratio is promised")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
