"""What logit rules, a guide and log-probs cost inside a verify step (fl_forward_verify_lp, verify_adjust_kernel), measured in ONE process
on one GPU.  Not a test.

  (a) the verify_adjust launch alone, between two events (fl_op_verify_adjust_time), for T = 8 and 16 rows at V = 32 000 and
      V = 152 064 in its three forms: rules only, a guide whose states allow ~1000 ids only, both;
  (b) one verify step of 8 rows on synthetic Mistral-7B bf16 behind a 512-token prompt: with rules + guide + top_n 5 log-probs
      (fl_forward_verify_lp) against the same step on a cache with none of them (fl_forward_verify: the parent commit's path, which
      this commit runs unchanged when the cache has neither rules nor a guide), and against the 8 ruled, guided decode steps with
      log-probs (fl_decode_sample_lp) the verify step stands for.

All settings alternate inside the process, the order reversed every other round; reported: the median of the rounds with min .. max;
every timed window is at least 0.25 s.  No ratio is promised; acceptance on real text cannot be measured with random weights.

    python tools/verify_adjust_cost.py [--rounds 7] [--out profiles/r18/verify_adjust_cost.txt]
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
ALLOWED = 1000                                         # ids per guide state
RULES = dict(repetition_penalty=1.1, frequency_penalty=0.3, presence_penalty=0.2)
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def med(xs, fmt="%.3f"):
    return (fmt + " (" + fmt + " .. " + fmt + ")") % (np.median(xs), min(xs), max(xs))


def automaton(V, n_states=4, seed=0):
    """n_states states of ~ALLOWED ids each; id j leads to state j % n_states"""
    rs = np.random.RandomState(seed)
    lists = [np.sort(rs.choice(V, ALLOWED, replace=False)).astype(np.uint32) for _ in range(n_states)]
    row_ptr = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.uint64)
    tokens = np.concatenate(lists).astype(np.uint32)
    return row_ptr, tokens, (tokens % n_states).astype(np.uint32), lists


def launch_alone(rounds):
    for V in (32000, 152064):
        rs = np.random.RandomState(V)
        rows = (rs.randn(16, V) * 2.5).astype(np.float32)
        ids = rs.randint(0, V, 16).astype(np.uint32)
        words = rs.randint(0, 4, V).astype(np.uint32)
        biases = np.zeros(V, np.float32)
        biases[rs.choice(V, 64, replace=False)] = 1.0
        scal = (RULES["repetition_penalty"], RULES["frequency_penalty"], RULES["presence_penalty"])
        row_ptr, tokens, nxt, _ = automaton(V)
        states = (np.arange(16) % 4).astype(np.uint32)
        forms = {"rules only": dict(words=words, biases=biases, scalars=scal),
                 "guide only (~%d ids)" % ALLOWED: dict(guide=(row_ptr, tokens, nxt), states=states),
                 "rules + guide": dict(words=words, biases=biases, scalars=scal, guide=(row_ptr, tokens, nxt), states=states)}
        settings = [(T, name) for T in (8, 16) for name in forms]

        def run(T, name, iters):
            kw = dict(forms[name])
            if "states" in kw:
                kw["states"] = kw["states"][:T]
            return fa.op_verify_adjust_time(rows[:T], ids[:T], iters, **kw) * 1e3

        iters = {s: max(8, int(WINDOW * 1e6 / run(s[0], s[1], 8)) + 1) for s in settings}
        res = {s: [] for s in settings}
        for rep in range(rounds):
            for s in (settings if rep % 2 == 0 else settings[::-1]):
                res[s].append(run(s[0], s[1], iters[s]))
        say("(a) V = %d: us per verify_adjust launch of T rows" % V)
        for T, name in settings:
            say("    T %2d  %-24s %s" % (T, name, med(res[T, name], "%.1f")))


def build(cfg):
    wts = bench.synth_device_weights(torch, cfg, torch.device("cuda", 0))
    gm = fa.Model(cfg, bench.as_fl_tensors(wts, 0), dtype="bf16")
    del wts
    torch.cuda.empty_cache()
    return gm


def verify_step(gm, cfg, prompt, T, rounds):
    V = cfg["vocab_size"]
    row_ptr, tokens, nxt, lists = automaton(V)
    guide = fa.Guide(gm, row_ptr, tokens, nxt)
    bare, full = gm.new_cache(T + 64), gm.new_cache(T + 64)
    first = gm.forward_argmax(bare, prompt, 0)
    assert gm.forward_argmax(full, prompt, 0) == first
    bias = {int(j): 1.0 for j in np.random.RandomState(7).choice(V, 64, replace=False)}

    def install():
        full.set_logit_rules(prompt_ids=prompt, logit_bias=bias, **RULES)
        full.set_guide(guide, 0)

    install()
    plain = gm.decode_sample(full, first, T, 7, 0.0, logprobs=5)[0]       # the ruled, guided continuation: a draft the guide can reach
    draft_bare = gm.decode_greedy(bare, first, T, 7)
    forms = ["bare cache, fl_forward_verify (the parent's path)", "rules + guide + top_n 5, fl_forward_verify_lp",
             "rules + guide + top_n 5, 8 steps of fl_decode_sample_lp"]

    def step(name):
        if name == forms[0]:
            bare.truncate(T)
            gm.forward_verify(bare, first, draft_bare, T)
            return
        full.truncate(T)
        install()                                       # the table and the state as before the step (one small copy; part of every form's window)
        if name == forms[1]:
            gm.forward_verify_lp(full, first, plain, T, logprobs=5)
        else:
            gm.decode_sample(full, first, T, 8, 0.0, logprobs=5)

    def install_only():
        full.truncate(T)
        install()
        gm.synchronize()

    timed = forms + ["(the re-install alone, inside the two ruled windows)"]
    fn = {name: (lambda n=name: step(n)) for name in forms}
    fn[timed[-1]] = install_only
    reps = {}
    for name in timed:
        fn[name]()
        gm.synchronize()
        t0 = time.perf_counter()
        for _ in range(8):
            fn[name]()
        gm.synchronize()
        reps[name] = max(8, int(WINDOW / ((time.perf_counter() - t0) / 8)) + 1)
    res = {name: [] for name in timed}
    for rep in range(rounds):
        for name in (timed if rep % 2 == 0 else timed[::-1]):
            gm.synchronize()
            t0 = time.perf_counter()
            for _ in range(reps[name]):
                fn[name]()
            gm.synchronize()
            res[name].append((time.perf_counter() - t0) / reps[name] * 1e3)
    say("(b) one verify step of 8 rows behind a %d-token prompt, ms per call (forward + adjust + selection + scoring + copy-back + sync):" % T)
    g = np.median(res[forms[0]])
    for name in timed:
        say("    %-58s %s   x%.4f of the bare step" % (name, med(res[name]), np.median(res[name]) / g))
    for c in (bare, full):
        c.close()
    guide.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--prompt", type=int, default=512)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.rounds >= 7
    say("verify step with rules, guide and log-probs: cost on one GPU, %d rounds per setting, settings interleaved in one process, median (min .. max)" % a.rounds)
    launch_alone(a.rounds)
    cfg = MODEL_CONFIGS["mistral-7b"]
    gm = build(cfg)
    prompt = np.random.RandomState(1234).randint(0, cfg["vocab_size"], size=a.prompt).astype(np.uint32)
    prompt[0] = 1
    say("mistral-7b (random weights, bf16), V = %d" % cfg["vocab_size"])
    verify_step(gm, cfg, prompt, a.prompt, a.rounds)
    say("acceptance on real text was not and cannot be measured with random weights; no ratio is promised")
    gm.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
