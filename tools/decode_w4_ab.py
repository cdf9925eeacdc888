"""bf16, FP8 (e4m3 + row scale) and MXFP4 (e2m1 + e8m0 per 32) decode inside ONE process (same box, same clock history), on the
pattern of tools/decode_w8_ab.py.
(a) The whole decode loop: the three models are built from the same synthetic weights; every sample is a fresh cache (so a fresh
    hipGraph capture), the same prompt, K greedy steps timed; the three modes alternate, rotating the order every round; median and
    min..max of the rounds.
(b) The launch alone: fl_op_gemv_w4(iters=) beside fl_op_gemv_w8 on the model's five projection shapes, over rotating copies of the
    weights (HBM, not cache): microseconds per launch and bytes/s of each kernel's OWN bytes.
usage: python tools/decode_w4_ab.py [model prompt steps]...      (default: mistral-7b 512 256, tinyllama-1.1b 512 256)
       W4_AB_REPS=5 rounds; W4_AB_ITERS=200 launches per timing; W4_AB_LAUNCH=0 skips (b)"""
import json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch, bench
import fastllm_amd as fa
from fastllm_amd.configs import MODEL_CONFIGS

args = sys.argv[1:]
runs = [(args[i], int(args[i + 1]), int(args[i + 2])) for i in range(0, len(args) - 2, 3)] or [("mistral-7b", 512, 256), ("tinyllama-1.1b", 512, 256)]
REPS = int(os.environ.get("W4_AB_REPS", "5"))
ITERS = int(os.environ.get("W4_AB_ITERS", "200"))
LAUNCH = os.environ.get("W4_AB_LAUNCH", "1") != "0"
MODES = ("bf16", "fp8", "mxfp4")


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


def launches(cfg):
    """(name, N, K, epilogue) of the step's five projection shapes; gate/up as the hook takes it: 2 I rows in HF order."""
    h, I, V = cfg["hidden_size"], cfg["intermediate_size"], cfg["vocab_size"]
    d = h // cfg["num_attention_heads"]
    return [("qkv", (cfg["num_attention_heads"] + 2 * cfg["num_key_value_heads"]) * d, h, 0), ("o_proj", h, h, 0), ("gate_up", 2 * I, h, 1),
            ("down_proj", h, I, 0), ("lm_head", V, h, 0)]


def time_launch(N, K, epi):
    rs = np.random.RandomState(N + K)
    x = (rs.randint(-2, 3, size=K).astype(np.float32).view(np.uint32) >> 16).astype(np.uint16)        # small integers: exact bf16
    q8 = rs.randint(0, 120, size=(N, K)).astype(np.uint8)
    s8 = np.full(N, 2.0 ** -9, dtype=np.float32)
    q4 = rs.randint(0, 256, size=(N, K // 2)).astype(np.uint8)
    e4 = np.full((N, K // 32), 118, dtype=np.uint8)
    _, ms8 = fa.op_gemv_w8(x, q8, s8, epilogue=epi, iters=ITERS)
    _, ms4 = fa.op_gemv_w4(x, q4, e4, epilogue=epi, iters=ITERS)
    return ms8 * 1e3, N * K + 4 * N, ms4 * 1e3, N * (K // 2 + K // 32)


for name, T, K in runs:
    cfg = MODEL_CONFIGS[name]
    wts = bench.synth_device_weights(torch, cfg, torch.device("cuda", 0))
    tens = bench.as_fl_tensors(wts, 0)
    models = {"bf16": fa.Model(cfg, tens, dtype="bf16"), "fp8": fa.Model(cfg, tens, dtype="bf16", decode_weights="e4m3"),
              "mxfp4": fa.Model(cfg, tens, dtype="bf16", decode_weights="mxfp4")}
    del wts, tens; torch.cuda.empty_cache()
    prompt = np.random.RandomState(1234).randint(0, cfg["vocab_size"], size=T).astype(np.uint32)
    prompt[0] = 1
    res = {m: [] for m in MODES}
    for rep in range(REPS):
        for i in range(3):
            mode = MODES[(rep + i) % 3]
            res[mode].append(sample(models[mode], prompt, T, K))
    info = {k: m.info() for k, m in models.items()}
    out = dict(model=name, prompt=T, steps=K, reps=REPS)
    for m in MODES:
        med = float(np.median(res[m]))
        out[m] = dict(ms_per_step=round(med, 4), tokens_per_s=round(1e3 / med, 1), range_ms=[round(min(res[m]), 4), round(max(res[m]), 4)],
                      range_tokens_per_s=[round(1e3 / max(res[m]), 1), round(1e3 / min(res[m]), 1)],
                      weight_bytes_per_token=info[m].weight_bytes_per_token, hbm_bytes_allocated=info[m].hbm_bytes_allocated)
    print(json.dumps(out), flush=True)
    for m in models.values():
        m.close()
    del models
    if LAUNCH:
        print("%-10s %7s %7s   |   %10s %9s   |   %10s %9s   |  %s" % (name, "N", "K", "w8 us", "TB/s", "w4 us", "TB/s", "w8 / w4 time"))
        for lname, N, Kp, epi in launches(cfg):
            us8, by8, us4, by4 = time_launch(N, Kp, epi)
            print("%-10s %7d %7d   |   %10.2f %9.2f   |   %10.2f %9.2f   |  %.3f" % (lname, N, Kp, us8, by8 / us8 * 1e-6, us4, by4 / us4 * 1e-6, us8 / us4), flush=True)
