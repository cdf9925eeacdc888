"""bf16 decode against FP8 (e4m3 + row scale) decode inside ONE process (same box, same clock history), on the pattern of
tools/decode_ab.py: both models are built from the same synthetic weights, every sample is a fresh cache (so a fresh hipGraph
capture), the same prompt, K greedy steps timed, samples interleaved A B / B A, medians reported.  Then one eager, profiled decode
step of each model: per-launch time and achieved TB/s of the projection kernels (fl_profile_begin / _end), bf16 next to FP8.
usage: python tools/decode_w8_ab.py [model prompt steps]...      (default: mistral-7b 512 256, tinyllama-1.1b 128 128, qwen2-7b 4096 128)
       W8_AB_REPS=6 samples per model and mode; W8_AB_PROFILE=0 skips the per-launch table"""
import json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch, bench
import fastllm_amd as fa
from fastllm_amd.configs import MODEL_CONFIGS

args = sys.argv[1:]
runs = [(args[i], int(args[i + 1]), int(args[i + 2])) for i in range(0, len(args) - 2, 3)] or [("mistral-7b", 512, 256), ("tinyllama-1.1b", 128, 128), ("qwen2-7b", 4096, 128)]
REPS = int(os.environ.get("W8_AB_REPS", "6"))
PROFILE = os.environ.get("W8_AB_PROFILE", "1") != "0"


def sample(gm, prompt, T, K):
    c = gm.new_cache(T + K + 96)
    first = gm.forward_argmax(c, prompt, 0)
    t = gm.decode_greedy(c, first, T, 16)                      # warm-up + capture
    gm.synchronize(); t0 = time.perf_counter()
    gm.decode_greedy(c, int(t[-1]), T + 16, K)
    gm.synchronize()
    dt = time.perf_counter() - t0
    c.close()
    return dt / K * 1e3


def profile_step(gm, prompt, T, steps=8):
    c = gm.new_cache(T + steps + 96)
    tok = gm.forward_argmax(c, prompt, 0)
    tok = gm.forward_argmax(c, [tok], T)                       # (first eager step outside the profile)
    gm.profile_begin()
    for i in range(steps):
        tok = gm.forward_argmax(c, [tok], T + 1 + i)
    st = gm.profile_end()
    c.close()
    return {s["name"]: (s["total_ms"] / s["launches"] * 1e3, s["bytes"] / s["launches"], s["launches"] // steps) for s in st}


for name, T, K in runs:
    cfg = MODEL_CONFIGS[name]
    wts = bench.synth_device_weights(torch, cfg, torch.device("cuda", 0))
    tens = bench.as_fl_tensors(wts, 0)
    models = {"bf16": fa.Model(cfg, tens, dtype="bf16"), "fp8": fa.Model(cfg, tens, dtype="bf16", decode_weights="e4m3")}
    del wts, tens; torch.cuda.empty_cache()
    prompt = np.random.RandomState(1234).randint(0, cfg["vocab_size"], size=T).astype(np.uint32)
    prompt[0] = 1
    res = {"bf16": [], "fp8": []}
    for rep in range(REPS):
        for mode in ("bf16", "fp8") if rep % 2 == 0 else ("fp8", "bf16"):
            res[mode].append(sample(models[mode], prompt, T, K))
    ma, mb = float(np.median(res["bf16"])), float(np.median(res["fp8"]))
    info = {k: m.info() for k, m in models.items()}
    out = dict(model=name, prompt=T, steps=K, reps=REPS,
               bf16_ms_per_step=round(ma, 4), fp8_ms_per_step=round(mb, 4), bf16_tokens_per_s=round(1e3 / ma, 1), fp8_tokens_per_s=round(1e3 / mb, 1),
               speedup=round(ma / mb, 4), bf16_range_ms=[round(min(res["bf16"]), 4), round(max(res["bf16"]), 4)],
               fp8_range_ms=[round(min(res["fp8"]), 4), round(max(res["fp8"]), 4)],
               weight_bytes_per_token=dict(bf16=info["bf16"].weight_bytes_per_token, fp8=info["fp8"].weight_bytes_per_token),
               hbm_bytes_allocated=dict(bf16=info["bf16"].hbm_bytes_allocated, fp8=info["fp8"].hbm_bytes_allocated))
    print(json.dumps(out), flush=True)
    if PROFILE:
        prof = {k: profile_step(m, prompt, T) for k, m in models.items()}
        print("%-34s %5s %10s %9s   |   %-38s %10s %9s" % ("bf16 launch", "/step", "us", "TB/s", "fp8 launch", "us", "TB/s"))
        for n16, (us, by, per) in sorted(prof["bf16"].items()):
            if not n16.startswith("gemv"):
                continue
            n8 = n16[:-1] + ",w8]"
            us8, by8, _ = prof["fp8"].get(n8, (float("nan"), float("nan"), 0))
            print("%-34s %5d %10.2f %9.2f   |   %-38s %10.2f %9.2f" % (n16, per, us, by / us * 1e-6, n8, us8, by8 / us8 * 1e-6), flush=True)
        for k in ("bf16", "fp8"):
            other = sum(us * per for n, (us, by, per) in prof[k].items() if not n.startswith("gemv"))
            proj = sum(us * per for n, (us, by, per) in prof[k].items() if n.startswith("gemv"))
            print("%s eager step: projections %.1f us, everything else %.1f us" % (k, proj, other), flush=True)
    for m in models.values():
        m.close()
    del models
