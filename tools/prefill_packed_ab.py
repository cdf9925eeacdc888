"""Packed prefill (fl_batch_prefill) against the sequential single-sequence path, measured inside ONE process with the two sides
alternating and medians reported (tools/prefill_ab.py's method).  Synthetic Mistral-7B bf16 (as bench.py builds it).

1. n prompts of one length: (a) n fl_forward_sample calls on n fresh caches, one after the other; (b) one fl_batch_prefill of the same
   prompts on n fresh caches.  n in {2, 8, 32} x length in {8, 16, 64, 256}, and one ragged set of 32 lengths in 4..200.  Every shape is
   warmed first; a sample is a window of at least 0.25 s of back-to-back repetitions, host to host behind a synchronise.
2. The StreamBatcher scenario of the README (64 requests of 128 + 128 tokens through 32 slots) with PackedAdmit off, on with its
   defaults (max_tokens 2048) and on with max_tokens 4096 (the 32 admissions of a step in one call).

usage: prefill_packed_ab.py [shapes] [batcher]     (default: both)"""
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402  (its HIP runtime must initialise before the product library's)
torch.cuda.is_available()
import bench  # noqa: E402
import fastllm_amd as fa  # noqa: E402
from fastllm_amd.configs import MODEL_CONFIGS  # noqa: E402

REPS, WINDOW = 5, 0.25
what = set(sys.argv[1:]) or {"shapes", "batcher"}


def med(xs):
    return float(np.median(xs)), float(min(xs)), float(max(xs))


def window(f, sync):
    """ms per call of f over a window of at least WINDOW seconds"""
    f(); sync()
    n, t0 = 0, time.perf_counter()
    while True:
        f(); n += 1
        if n % 2 == 0 or n == 1:
            sync()
            dt = time.perf_counter() - t0
            if dt >= WINDOW:
                return dt / n * 1e3


def shapes(gm, cfg):
    rs = np.random.RandomState(0)
    sets = [("n=%2d x %3d" % (n, T), [T] * n) for n in (2, 8, 32) for T in (8, 16, 64, 256)]
    sets.append(("ragged 32 x 4..200", [int(x) for x in rs.randint(4, 201, size=32)]))
    work = []
    for label, lens in sets:
        prompts = [rs.randint(0, cfg["vocab_size"], size=T).astype(np.uint32) for T in lens]
        caches = [gm.new_cache(max(lens) + 8) for _ in lens]

        def single(prompts=prompts, caches=caches):
            for c, p in zip(caches, prompts):
                c.reset()
                gm.forward_sample(c, p, 0, 0.0)

        def packed(prompts=prompts, caches=caches):
            for c in caches:
                c.reset()
            gm.prefill_packed(caches, prompts)
        single(); packed(); gm.synchronize()                    # warm-up of every shape before anything is timed
        work.append((label, lens, single, packed, caches))
    print("# %s bf16 synthetic; (a) n single prefills one after the other, (b) one packed prefill; ms per set, median (min..max) of %d windows >= %.2f s"
          % ("mistral-7b", REPS, WINDOW))
    for label, lens, single, packed, caches in work:
        res = {"a": [], "b": []}
        for rep in range(REPS):
            for side in ("a", "b") if rep % 2 == 0 else ("b", "a"):
                res[side].append(window(single if side == "a" else packed, gm.synchronize))
        (am, alo, ahi), (bm, blo, bhi) = med(res["a"]), med(res["b"])
        print("%-20s %5d tokens: (a) %8.3f ms (%.3f..%.3f)   (b) %8.3f ms (%.3f..%.3f)   b/a %.3f%s"
              % (label, sum(lens), am, alo, ahi, bm, blo, bhi, bm / am, "   PACKED SLOWER" if bm > am else ""), flush=True)
        for c in caches:
            c.close()


def batcher(gm, cfg, slots=32, requests=64, prompt=128, gen=128):
    host = C.CDLL(os.path.join(ROOT, "fastllm_amd", "lib", "libfastllm_host.so"))
    host.flh_last_error.restype = C.c_char_p
    TOK = C.CFUNCTYPE(C.c_int, C.c_uint64, C.c_uint32, C.c_void_p)
    DONE = C.CFUNCTYPE(None, C.c_uint64, C.c_size_t, C.c_void_p)
    sz = C.c_size_t
    host.flh_batcher_create_on_packed.argtypes = [C.c_void_p, sz, sz, sz, C.c_int, C.c_int, sz, sz, C.POINTER(C.c_void_p)]
    host.flh_batcher_submit.argtypes = [C.c_void_p, C.c_void_p, sz, sz, C.c_float, C.c_int64, TOK, DONE, C.c_void_p, C.POINTER(C.c_uint64)]
    host.flh_batcher_run.argtypes = [C.c_void_p, C.POINTER(sz), C.POINTER(sz)]
    host.flh_batcher_packed_stats.argtypes = [C.c_void_p, C.POINTER(sz), C.POINTER(sz)]
    host.flh_batcher_destroy.argtypes = [C.c_void_p]
    count = [0]

    def on_token(_rid, _tok, _u):
        count[0] += 1
        return 1
    cb, dcb = TOK(on_token), DONE(lambda _rid, _n, _u: None)
    rs = np.random.RandomState(1)
    prompts = [rs.randint(0, cfg["vocab_size"], size=prompt).astype(np.uint32) for _ in range(requests)]

    def once(max_tokens):                                        # 0: PackedAdmit off
        b = C.c_void_p()
        if host.flh_batcher_create_on_packed(gm._h, slots, prompt + gen + 16, 16, 0, 1 if max_tokens else 0, 256, max_tokens, C.byref(b)) != 0:
            raise RuntimeError(host.flh_last_error().decode(errors="replace"))
        count[0] = 0
        t0 = time.perf_counter()
        for p in prompts:
            rid = C.c_uint64(0)
            if host.flh_batcher_submit(b, p.ctypes.data, p.size, gen, 0.0, -1, cb, dcb, None, C.byref(rid)) != 0:
                raise RuntimeError(host.flh_last_error().decode(errors="replace"))
        steps, pre, calls, pk = sz(0), sz(0), sz(0), sz(0)
        rc = host.flh_batcher_run(b, C.byref(steps), C.byref(pre))
        dt = time.perf_counter() - t0
        host.flh_batcher_packed_stats(b, C.byref(calls), C.byref(pk))
        host.flh_batcher_destroy(b)
        if rc != 0:
            raise RuntimeError(host.flh_last_error().decode(errors="replace"))
        return count[0] / dt, dt, steps.value, pre.value, calls.value, pk.value
    sides = (0, 2048, 4096)                                      # off; on with the default max_tokens; on with a step's 32 admissions in one call
    for side in sides:
        once(side)                                               # (the first passes capture the step's graph)
    res = {side: [] for side in sides}
    for rep in range(REPS):
        for side in sides if rep % 2 == 0 else sides[::-1]:
            res[side].append(once(side))
    print("# StreamBatcher, %d requests of %d + %d tokens through %d slots (PackedAdmit max_prompt 256); tokens/s, median (min..max) of %d runs"
          % (requests, prompt, gen, slots, REPS))
    off = med([r[0] for r in res[0]])[0]
    for side in sides:
        m, lo, hi = med([r[0] for r in res[side]])
        r = res[side][0]
        print("PackedAdmit %-20s %8.1f tokens/s (%.1f..%.1f)   x %.3f   batch steps %d, prefills %d in %d calls (%d packed)"
              % ("max_tokens %d" % side if side else "off", m, lo, hi, m / off, r[2], r[3], r[4], r[5]), flush=True)


name = "mistral-7b"
cfg = MODEL_CONFIGS[name]
wts = bench.synth_device_weights(torch, cfg, torch.device("cuda", 0))
gm = fa.Model(cfg, bench.as_fl_tensors(wts, 0), dtype="bf16")
del wts
torch.cuda.empty_cache()
if "shapes" in what:
    shapes(gm, cfg)
if "batcher" in what:
    batcher(gm, cfg)
