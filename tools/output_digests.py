#!/usr/bin/env python3
"""One sha256 per output array of the attention paths a refactor of the prefill attention / RoPE kernels must leave bit-identical,
written as JSON {name: digest}.  Run it once per library (FL_LIB_PATH), each in a fresh process, and compare the files:

    python tools/output_digests.py OUT.json                 (writes)
    python tools/output_digests.py compare A.json B.json     (exit status 0: same names, same digests)

Arrays: every case of tests/test_gpu_attention_ops.py::test_prefill_kernels with kernel=2; every pack of
tests/test_gpu_packed_attention.py's PACKS at its five head shapes and both head sizes (all members in one launch); and for every
tests/synth.py config in bf16 and fp32: the logits of a 5-token prompt, the ids of 8 greedy decode steps, the ids of batches of 3
and 9 streams, and the tokens and logits of one prefill_packed of three prompts."""
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)


def digest(a):
    a = np.ascontiguousarray(a)
    return hashlib.sha256(str((a.dtype.str, a.shape)).encode() + a.tobytes()).hexdigest()


def collect():
    import fastllm_amd as fa
    import synth
    import test_gpu_attention_ops as ops
    import test_gpu_packed_attention as pk
    out = {}
    for d in (64, 128):
        for H, Hkv in ops.GROUPS:
            for T, s_past, window in ops.PREFILL_CASES:
                q, k, v = ops.prefill_inputs(T, s_past, H, Hkv, d, 2)
                out["prefill16/d%d/H%d_%d/T%d_%d_w%d" % (d, H, Hkv, T, s_past, window)] = digest(fa.op_attention(q, k, v, s_past, H, Hkv, d, window=window, kernel=2))
    for pack in pk.PACKS:
        for H, Hkv in pk.SHAPES:
            for d in (64, 128):
                c = pk.case(pack, H, Hkv, d)
                got = pk.run(fa, c, list(range(len(c[0]))), H, Hkv, d)
                out["packed/%s/d%d/H%d_%d" % (pack, d, H, Hkv)] = digest(np.concatenate([got[i] for i in range(len(c[0]))]))
    for name, cfg in synth.CONFIGS.items():
        w = synth.synth_weights(cfg)
        for dtype in ("bf16", "f32"):
            gm = fa.Model(cfg, w, dtype=dtype)
            key = "model/%s/%s/" % (name, dtype)
            ids = synth.prompt_ids(cfg, 5)
            c = gm.new_cache(64)
            out[key + "logits5"] = digest(gm.forward(c, ids, 0))
            c2 = gm.new_cache(64)
            first = gm.forward_argmax(c2, ids, 0)
            out[key + "ids8"] = digest(np.concatenate([[first], gm.decode_greedy(c2, first, len(ids), 8)]).astype(np.uint32))
            for B in (3, 9):
                caches, toks, lens = [], [], []
                for i in range(B):
                    p = synth.prompt_ids(cfg, 3 + i % 5, seed=50 + i)
                    cc = gm.new_cache(64)
                    toks.append(gm.forward_argmax(cc, p, 0)); lens.append(len(p)); caches.append(cc)
                batch = fa.Batch(gm, caches)
                out[key + "batch%d" % B] = digest(np.asarray(batch.decode(toks, lens, 6)).astype(np.uint32))
                batch.close()
            prompts = [synth.prompt_ids(cfg, n, seed=700 + i) for i, n in enumerate((17, 5, 48))]
            pc = [gm.new_cache(64) for _ in prompts]
            toks, lg = gm.prefill_packed(pc, prompts, want_logits=True)
            out[key + "packed3/tokens"] = digest(np.asarray(toks).astype(np.uint32))
            for i, row in enumerate(lg):
                out[key + "packed3/logits%d" % i] = digest(row)
            gm.close()
    return out


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "compare":
        a, b = (json.load(open(p)) for p in sys.argv[2:4])
        diff = sorted(k for k in set(a) | set(b) if a.get(k) != b.get(k))
        print("%d arrays compared, %d differ" % (len(set(a) | set(b)), len(diff)))
        for k in diff:
            print("  " + k)
        sys.exit(1 if diff else 0)
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    res = collect()
    with open(sys.argv[1], "w") as f:
        json.dump(res, f, indent=0, sort_keys=True)
    print("%d arrays -> %s" % (len(res), sys.argv[1]))
