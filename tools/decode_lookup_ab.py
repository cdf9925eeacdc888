"""Cost of the verify step and speed of the prompt-lookup loop against the plain greedy loop, inside ONE process (same box, same
clock history; samples of the forms interleaved; medians with spread).
usage: python tools/decode_lookup_ab.py [model] [prompt] [steps] [out.txt]

  1. ms per fl_forward_verify step at n_draft = 0, 1, 3, 7, 15 (drafts = the model's own continuation, so every row is accepted and
     the cache moves as in the loop) against the ms of a decode step of fl_decode_greedy;
  2. tokens/s of fl_decode_lookup against fl_decode_greedy on the same prompt, with a corpus that CONTAINS the true continuation
     (prompt ++ [first] ++ greedy output), clean and corrupted at every c-th id for c = 8, 4, 2: speed at FORCED acceptance.

No real checkpoint exists for these measurements: the weights are random, greedy loops of random-weight models fall into cycles
(which flatters lookup), and acceptance on real text cannot be measured.  So this reports cost per step and speed at forced
acceptance, never a "typical" speed-up."""
import os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch, bench
import fastllm_amd as fa
from fastllm_amd.configs import MODEL_CONFIGS
name = sys.argv[1] if len(sys.argv) > 1 else "mistral-7b"
T = int(sys.argv[2]) if len(sys.argv) > 2 else 512
K = int(sys.argv[3]) if len(sys.argv) > 3 else 256
OUT = sys.argv[4] if len(sys.argv) > 4 else None
REPS = 5
cfg = MODEL_CONFIGS[name]
wts = bench.synth_device_weights(torch, cfg, torch.device("cuda", 0))
gm = fa.Model(cfg, bench.as_fl_tensors(wts, 0), dtype="bf16")
del wts; torch.cuda.empty_cache()
V = cfg["vocab_size"]
prompt = np.random.RandomState(1234).randint(0, V, size=T).astype(np.uint32)
prompt[0] = 1
lines = []
def say(s):
    print(s, flush=True)
    lines.append(s)
def fresh():
    c = gm.new_cache(T + K + 96)
    return c, gm.forward_argmax(c, prompt, 0)
def med(xs):
    return "%.3f (%.3f..%.3f)" % (np.median(xs), min(xs), max(xs))

c, first = fresh()
want = gm.decode_greedy(c, first, T, K)
c.close()
say("%s bf16, prompt %d, %d steps; greedy output has %d distinct ids of %d" % (name, T, K, len(set(want.tolist())), K))

# ---- 1. cost per step -------------------------------------------------------------------------------------------------------
NDS = [0, 1, 3, 7, 15]
STEPS = 12                                             # verify steps timed per sample (the cache moves by n_draft + 1 each)
ms = {nd: [] for nd in NDS}
ms_dec, acc = [], {nd: [] for nd in NDS}
for rep in range(REPS):
    order = NDS if rep % 2 == 0 else NDS[::-1]
    c, f = fresh()
    t = gm.decode_greedy(c, f, T, 16)                  # warm-up + capture
    gm.synchronize(); t0 = time.perf_counter()
    gm.decode_greedy(c, int(t[-1]), T + 16, 64)
    gm.synchronize()
    ms_dec.append((time.perf_counter() - t0) / 64 * 1e3)
    c.close()
    for nd in order:
        c, f = fresh()
        seq = np.concatenate([[f], want])
        i = 0
        gm.forward_verify(c, int(seq[0]), seq[1:1 + nd], T); i += len(c) - T     # warm-up (scratch, buffers)
        n0 = i
        gm.synchronize(); t0 = time.perf_counter()
        for _ in range(STEPS):
            toks, _ = gm.forward_verify(c, int(seq[i]), seq[i + 1:i + 1 + nd], T + i)
            i += len(toks)
        gm.synchronize()
        ms[nd].append((time.perf_counter() - t0) / STEPS * 1e3)
        acc[nd].append((i - n0) / STEPS - 1)
        c.close()
d = np.median(ms_dec)
say("decode step (fl_decode_greedy, graph replay): %s ms" % med(ms_dec))
for nd in NDS:
    say("verify step n_draft %2d: %s ms = %.3f decode steps; accepted %.2f of %d per step" % (nd, med(ms[nd]), np.median(ms[nd]) / d, np.mean(acc[nd]), nd))

# ---- 2. the loop at forced acceptance ----------------------------------------------------------------------------------------
def corpus_of(cth):
    w = want.copy()
    if cth:
        w[cth - 1::cth] = (w[cth - 1::cth] + 1) % V
    return np.concatenate([prompt, [first], w]).astype(np.uint32)
FORMS = [("greedy", None), ("lookup clean", 0), ("lookup c=8", 8), ("lookup c=4", 4), ("lookup c=2", 2)]
tps = {k: [] for k, _ in FORMS}
stats, equal = {}, {}
for rep in range(REPS):
    for k, cth in FORMS if rep % 2 == 0 else FORMS[::-1]:
        c, f = fresh()
        if cth is None:
            t = gm.decode_greedy(c, f, T, 16); c.truncate(T)           # warm-up + capture, then back to the prompt
            gm.decode_greedy(c, f, T, 16); c.truncate(T)
            gm.synchronize(); t0 = time.perf_counter()
            got = gm.decode_greedy(c, f, T, K)
        else:
            gm.decode_lookup(c, corpus_of(cth), f, T, 32); c.truncate(T)
            gm.synchronize(); t0 = time.perf_counter()
            got, stats[k] = gm.decode_lookup(c, corpus_of(cth), f, T, K, return_stats=True)
        gm.synchronize()
        tps[k].append(K / (time.perf_counter() - t0))
        equal[k] = bool(np.array_equal(got, want))
        c.close()
g = np.median(tps["greedy"])
for k, cth in FORMS:
    extra = ""
    if cth is not None:
        s = stats[k]
        extra = "   x%.3f of greedy; %d steps, %d drafted, %d accepted (%.2f per step); ids equal greedy: %s" % (
            np.median(tps[k]) / g, s["steps"], s["drafted"], s["accepted"], s["accepted"] / max(1, s["steps"]), equal[k])
    say("%-13s %s tokens/s%s" % (k, med(tps[k]), extra))
if OUT:
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    open(OUT, "w").write("\n".join(lines) + "\n")
