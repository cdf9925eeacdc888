"""What decoder-model embeddings (fl_batch_embed) cost, measured in ONE process on random weights in bf16.

(a) the pool launch alone, between events (fl_op_pool_rows_time), at h = 4096: 64 members x 128 rows and 1 member x 8192 rows, LAST
    and MEAN, with and without the normalising second launch; a sample is a window of at least 0.25 s of launches.
(b) Mistral-7B-shaped: fl_batch_embed (LAST, causal, normalised) against fl_batch_prefill of the same pack (the path every earlier
    commit runs, the yardstick) at 32 x 64 tokens and 8 x 512 tokens.  The embed call leaves out the lm_head of n rows and the token
    selection and adds the final norm over all rows and the pool launch.
(c) FL_MASK_FULL against FL_MASK_CAUSAL on the 8 x 512 pack.

(b), (c): the settings are interleaved round by round (so drift hits them alike), the order reversed every other round; every sample
is a window of whole calls on reset caches lasting at least 0.25 s, closed by a synchronise; reported: the median ms per call over
the rounds with the min .. max spread.

    python tools/embed_decoder_cost.py [--rounds 5] [--window 0.25] [--out profiles/r17/embed_decoder.txt]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import score_cost as sc  # noqa: E402  (torch first, the shared window / interleave / report helpers)
import fastllm_amd as fa  # noqa: E402
from fastllm_amd.configs import MODEL_CONFIGS  # noqa: E402

say = sc.say


def part_a(rounds, seconds):
    say("(a) the pool launch(es) alone at h = 4096, ms per pool between events, windows of at least %.2f s (median of %d, min .. max)" % (seconds, rounds))
    rs = np.random.RandomState(1)
    h = 4096
    w = (1.0 + 0.1 * rs.standard_normal(h)).astype(np.float32)
    for n, rows in ((64, 128), (1, 8192)):
        x = rs.standard_normal((n * rows, h)).astype(np.float32)
        inv = rs.uniform(0.5, 2.0, n * rows).astype(np.float32)
        for pooling in ("last", "mean"):
            for normalize in (False, True):
                # every sample a window of at least `seconds` of back-to-back launches between the two events (sized by a short run)
                first = fa.op_pool_rows(x, inv, w, [rows] * n, pooling=pooling, normalize=normalize, iters=64)
                iters = int(min(1 << 20, max(64, np.ceil(seconds * 1e3 / max(first, 1e-4)))))
                v = np.array([fa.op_pool_rows(x, inv, w, [rows] * n, pooling=pooling, normalize=normalize, iters=iters) for _ in range(rounds)])
                m = np.median(v)
                read = (n * rows if pooling == "mean" else n) * h * 4
                say("  %2d x %4d rows %-4s normalize=%d   %8.4f ms  (min %.4f .. max %.4f)   %7.1f GB/s of row reads"
                    % (n, rows, pooling, normalize, m, v.min(), v.max(), read / (m * 1e-3) / 1e9))


def pack_settings(gm, V, n, T, masks):
    rs = np.random.RandomState(99)
    seqs = [rs.randint(0, V, size=T).astype(np.uint32) for _ in range(n)]
    caches = [gm.new_cache(T + 32) for _ in range(n)]

    def reset():
        for c in caches:
            c.reset()

    def prefill():
        reset(); gm.prefill_packed(caches, seqs)

    def embed(mask):
        def f():
            reset(); gm.embed_packed(caches, seqs, pooling="last", mask=mask, normalize=True)
        return f

    s = [("fl_batch_prefill %d x %d" % (n, T), fa.reload_env, prefill)]
    for mask in masks:
        s.append(("fl_batch_embed %d x %d last %s" % (n, T, mask), fa.reload_env, embed(mask)))
    return s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.25)
    ap.add_argument("--out", default=None)
    ap.add_argument("--parts", default="abc")
    a = ap.parse_args()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").close()
        sc.OUT["path"] = a.out
    say("embed_decoder_cost: %d rounds, windows of at least %.2f s, one process" % (a.rounds, a.window))
    if "a" in a.parts:
        part_a(a.rounds, a.window)
    if "b" in a.parts or "c" in a.parts:
        cfg = MODEL_CONFIGS["mistral-7b"]
        gm = sc.build(cfg)
        V = cfg["vocab_size"]
        if "b" in a.parts:
            say("(b) mistral-7b (random weights, bf16): fl_batch_embed against fl_batch_prefill of the same pack, caches reset per call")
            for n, T in ((32, 64), (8, 512)):
                s = pack_settings(gm, V, n, T, ("causal",))
                sc.report(sc.interleaved(gm, s, a.rounds, a.window), s[0][0])
        if "c" in a.parts:
            say("(c) mistral-7b: FL_MASK_FULL against FL_MASK_CAUSAL, 8 x 512 tokens (the full mask does about twice the attention FLOPs)")
            s = pack_settings(gm, V, 8, 512, ("causal", "full"))[1:]
            sc.report(sc.interleaved(gm, s, a.rounds, a.window), s[0][0])
        gm.close()


if __name__ == "__main__":
    main()
