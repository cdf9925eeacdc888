"""What packed verify (fl_batch_verify, fl_batch_decode_lookup, StreamBatcher's BatchLookup) costs and saves, measured in ONE process
on one GPU: synthetic Mistral-7B bf16 behind 512-token prompts.  Not a test.

  (a) one packed verify step of n x (1 + d) rows, n in {2, 8, 32}, d in {3, 7, 15}, greedy and top-p 0.9, beside n single
      fl_forward_verify_ex calls, ONE step of fl_batch_decode_each_ex on the same n streams (what the packed step costs against at zero
      acceptance) and 1 + d such steps (what it replaces at full acceptance); break-even accepted drafts per stream per step =
      t_packed / t_step - 1;
  (b) fl_batch_decode_lookup at FORCED acceptance (the corpus holds each member's own continuation, the method of
      tools/decode_lookup_ab.py) against fl_batch_decode_each_ex in tokens/s: the CEILING, never a typical speed-up;
  (c) the README's StreamBatcher scenario, 64 requests of 128 + 128 tokens through 32 slots, BatchLookup off and on: with random weights
      acceptance is near zero, so this is the WORST-CASE overhead of the option;
  (d) the selection kernel alone (fl_op_verify_packed, iters) at 256 rows, V = 32 000 and 152 064, ArgMax / top-p / top-k.

All settings of a part alternate inside the process, the order reversed every other round; reported: the median of the rounds with
min .. max; every timed window is at least 0.25 s.  Acceptance on real text cannot be measured with random weights.

    python tools/batch_verify_ab.py [--rounds 5] [--out profiles/r16/batch_verify.txt] [--parts abcd]
"""
import argparse
import ctypes as C
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


def timed(gm, fn):
    """ms per call of fn over a window of at least WINDOW seconds that ends in a synchronise"""
    gm.synchronize()
    t0 = time.perf_counter()
    n = 0
    while True:
        fn()
        n += 1
        if n % 2 == 0 or n == 1:
            gm.synchronize()
            if time.perf_counter() - t0 >= WINDOW:
                break
    gm.synchronize()
    return (time.perf_counter() - t0) / n * 1e3


def interleave(gm, forms, rounds):
    """forms: [(name, fn)]; returns {name: [ms per call, one per round]}"""
    for _, fn in forms:
        fn()                                           # warm-up: scratch, graphs, code objects
    gm.synchronize()
    res = {name: [] for name, _ in forms}
    for rep in range(rounds):
        for name, fn in (forms if rep % 2 == 0 else forms[::-1]):
            res[name].append(timed(gm, fn))
    return res


def build(cfg):
    wts = bench.synth_device_weights(torch, cfg, torch.device("cuda", 0))
    gm = fa.Model(cfg, bench.as_fl_tensors(wts, 0), dtype="bf16")
    del wts
    torch.cuda.empty_cache()
    return gm


def streams(gm, cfg, n, T, room):
    """n caches behind their own T-token prompts, every prompt's own first token"""
    cs, firsts, prompts = [], [], []
    for i in range(n):
        p = np.random.RandomState(1234 + i).randint(0, cfg["vocab_size"], size=T).astype(np.uint32)
        p[0] = 1
        c = gm.new_cache(T + room)
        firsts.append(gm.forward_argmax(c, p, 0))
        cs.append(c)
        prompts.append(p)
    return cs, firsts, prompts


def part_a(gm, cfg, T, rounds):
    say("(a) one step behind %d-token prompts, ms per step (forward + selection + copy-back + one synchronise); break-even = t_packed / t_step - 1" % T)
    say("     n   d  sampler   | packed verify        | n single verify calls | 1 batch step          | 1 + d batch steps     | break-even accepted / stream")
    for n in (2, 8, 32):
        cs, firsts, _ = streams(gm, cfg, n, T, 64)
        batch = fa.Batch(gm, cs)
        for d in (3, 7, 15):
            drafts = [np.random.RandomState(77 + i).randint(0, cfg["vocab_size"], size=d).astype(np.uint32) for i in range(n)]
            for sname, kw1, kwn in (("greedy", {}, {}), ("top-p 0.9", dict(temperature=0.8, top_p=0.9, seed=3, draws_done=1),
                                                   dict(temperatures=[0.8] * n, top_p=[0.9] * n, seeds=[3] * n, draws_done=[1] * n))):
                def back():
                    for c in cs:
                        c.truncate(T)                   # host state only: the same cache state for every call

                def packed():
                    gm.verify_packed(cs, firsts, drafts, [T] * n, **kwn)
                    back()

                def singles():
                    for i in range(n):
                        gm.forward_verify(cs[i], firsts[i], drafts[i], T, **kw1)
                    back()

                def steps(k):
                    def f():
                        batch.decode_each(firsts, [T] * n, k, **kwn)
                        back()
                    return f
                forms = [("packed", packed), ("singles", singles), ("step", steps(1)), ("steps", steps(1 + d))]
                r = interleave(gm, forms, rounds)
                be = np.median(r["packed"]) / np.median(r["step"]) - 1
                say("    %2d  %2d  %-9s | %s | %s | %s | %s | %.2f" % (n, d, sname, med(r["packed"]), med(r["singles"]), med(r["step"]), med(r["steps"]), be))
        batch.close()
        for c in cs:
            c.close()


def part_b(gm, cfg, T, K, rounds):
    say("(b) %d tokens per stream behind %d-token prompts, the corpus holds each member's own continuation (FORCED acceptance: the CEILING), tokens/s over all streams:" % (K, T))
    for n in (2, 8, 32):
        cs, firsts, prompts = streams(gm, cfg, n, T, K + 96)
        batch = fa.Batch(gm, cs)

        def back():
            for c in cs:
                c.truncate(T)
        plain = batch.decode_each(firsts, [T] * n, K)
        back()
        for md in (7, 15):
            # the corpus must hold the continuation THE LOOP ITSELF produces (bf16 rows of a multi-row call and one-row steps part at
            # near-ties, which random weights are full of): feed the loop its own output until it reproduces it
            cur = [np.asarray(p) for p in plain]
            for passes in range(1, 33):
                got = gm.decode_lookup_packed(cs, [np.concatenate([prompts[i], [firsts[i]], cur[i]]).astype(np.uint32) for i in range(n)], firsts, [T] * n,
                                              [K] * n, max_draft=md)
                back()
                same = all(np.array_equal(g, c) for g, c in zip(got, cur))
                cur = got
                if same:
                    break
            corpora = [np.concatenate([prompts[i], [firsts[i]], cur[i]]).astype(np.uint32) for i in range(n)]
            stats = {}

            def lookup():
                _, st = gm.decode_lookup_packed(cs, corpora, firsts, [T] * n, [K] * n, max_draft=md, return_stats=True)
                stats["st"] = st
                back()

            def each():
                batch.decode_each(firsts, [T] * n, K)
                back()
            r = interleave(gm, [("lookup", lookup), ("each", each)], rounds)
            tl, te = [n * K / (x / 1e3) for x in r["lookup"]], [n * K / (x / 1e3) for x in r["each"]]
            st = stats["st"]
            say("    n %2d max_draft %2d: fl_batch_decode_lookup %s | fl_batch_decode_each_ex %s | x%.3f; fixed point after %d pass(es): %s; member 0: %d steps, %d drafted, %d accepted"
                % (n, md, med(tl, "%.1f"), med(te, "%.1f"), np.median(tl) / np.median(te), passes, same, st[0]["steps"], st[0]["drafted"], st[0]["accepted"]))
        batch.close()
        for c in cs:
            c.close()


def part_c(gm, cfg, rounds, slots=32, requests=64, prompt=128, gen=128):
    host = C.CDLL(os.path.join(ROOT, "fastllm_amd", "lib", "libfastllm_host.so"))
    host.flh_last_error.restype = C.c_char_p
    TOK = C.CFUNCTYPE(C.c_int, C.c_uint64, C.c_uint32, C.c_void_p)
    DONE = C.CFUNCTYPE(None, C.c_uint64, C.c_size_t, C.c_void_p)
    sz = C.c_size_t
    host.flh_batcher_create_on_lookup.argtypes = [C.c_void_p, sz, sz, sz, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, sz, C.POINTER(C.c_void_p)]
    host.flh_batcher_lookup_stats.argtypes = [C.c_void_p, C.POINTER(sz), C.POINTER(sz), C.POINTER(sz)]
    host.flh_batcher_submit.argtypes = [C.c_void_p, C.c_void_p, sz, sz, C.c_float, C.c_int64, TOK, DONE, C.c_void_p, C.POINTER(C.c_uint64)]
    host.flh_batcher_run.argtypes = [C.c_void_p, C.POINTER(sz), C.POINTER(sz)]
    host.flh_batcher_destroy.argtypes = [C.c_void_p]
    count = [0]
    cb = TOK(lambda _r, _t, _u: count.__setitem__(0, count[0] + 1) or 1)
    dcb = DONE(lambda _r, _n, _u: None)
    prompts = [np.random.RandomState(500 + i).randint(0, cfg["vocab_size"], size=prompt).astype(np.uint32) for i in range(requests)]

    def run(on):
        b = C.c_void_p()
        if host.flh_batcher_create_on_lookup(gm._h, slots, prompt + gen + 16, 16, 0, on, 7, 3, 1, 1, C.byref(b)) != 0:
            raise RuntimeError(host.flh_last_error().decode(errors="replace"))
        count[0] = 0
        t0 = time.perf_counter()
        for p in prompts:
            rid = C.c_uint64(0)
            if host.flh_batcher_submit(b, p.ctypes.data, p.size, gen, 0.0, -1, cb, dcb, None, C.byref(rid)) != 0:
                raise RuntimeError(host.flh_last_error().decode(errors="replace"))
        steps, pre, v, d, a = sz(0), sz(0), sz(0), sz(0), sz(0)
        rc = host.flh_batcher_run(b, C.byref(steps), C.byref(pre))
        dt = time.perf_counter() - t0
        host.flh_batcher_lookup_stats(b, C.byref(v), C.byref(d), C.byref(a))
        host.flh_batcher_destroy(b)
        if rc != 0:
            raise RuntimeError(host.flh_last_error().decode(errors="replace"))
        return count[0] / dt, (steps.value, v.value, d.value, a.value)
    run(0), run(1)                                     # warm-up
    res, info = {0: [], 1: []}, {}
    for rep in range(rounds):
        for on in ((0, 1) if rep % 2 == 0 else (1, 0)):
            tps, info[on] = run(on)
            res[on].append(tps)
    say("(c) StreamBatcher, %d requests of %d + %d tokens through %d slots, prefills included, tokens/s (random weights: acceptance near zero, so this is the WORST-CASE overhead of the option):"
        % (requests, prompt, gen, slots))
    for on in (0, 1):
        s = info[on]
        say("    BatchLookup %-3s %s   x%.4f of off; %d batch steps, %d verify steps, %d drafted, %d accepted" % (
            "on" if on else "off", med(res[on], "%.1f"), np.median(res[on]) / np.median(res[0]), s[0], s[1], s[2], s[3]))


def part_d(rounds):
    say("(d) the selection launch alone (fl_op_verify_packed), 256 rows = 16 members x 16 rows in one launch, us per launch:")
    for V in (32000, 152064):
        lg = (np.random.RandomState(V).randn(256, V) * 2.5).astype(np.float32)
        members = [np.zeros(16, np.uint32)] * 16
        forms = [("ArgMax", {}), ("top-p 0.9 t=0.8", dict(temperatures=[0.8] * 16, top_p=[0.9] * 16)), ("top-k 40 t=0.8", dict(temperatures=[0.8] * 16, top_k=[40] * 16))]
        iters, res = {}, {name: [] for name, _ in forms}
        for name, kw in forms:
            ms = fa.op_verify_packed(lg, members, iters=4, **kw)[-1]
            iters[name] = max(4, int(WINDOW * 1e3 / ms) + 1)
        for rep in range(rounds):
            for name, kw in (forms if rep % 2 == 0 else forms[::-1]):
                res[name].append(fa.op_verify_packed(lg, members, iters=iters[name], **kw)[-1] * 1e3)
        for name, _ in forms:
            say("    V %6d  %-16s %s" % (V, name, med(res[name], "%.1f")))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--prompt", type=int, default=512)
    ap.add_argument("--steps", type=int, default=128)
    ap.add_argument("--parts", default="abcd")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.rounds >= 5
    say("packed verify: cost on one GPU, %d rounds per setting, settings interleaved in one process, median (min .. max), windows of at least 0.25 s" % a.rounds)
    if "d" in a.parts:
        part_d(a.rounds)
    if set("abc") & set(a.parts):
        cfg = MODEL_CONFIGS["mistral-7b"]
        gm = build(cfg)
        say("mistral-7b (random weights, bf16), V = %d" % cfg["vocab_size"])
        if "a" in a.parts:
            part_a(gm, cfg, a.prompt, a.rounds)
        if "b" in a.parts:
            part_b(gm, cfg, a.prompt, a.steps, a.rounds)
        if "c" in a.parts:
            part_c(gm, cfg, a.rounds)
        gm.close()
    say("acceptance on real text was not and cannot be measured with random weights: (b) is the speed when every draft is right, (c) when none is")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
