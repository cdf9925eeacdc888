"""Embedding throughput of the encoder (fl_encoder_embed) at the all-MiniLM-L6-v2 shape -- h 384, 12 heads, I 1536, 6 layers, V 30522,
P 512 -- with random weights generated on the device: sequences/s and ms per call for one sequence of 16 and of 128 tokens, 64 x 128
and 256 ragged sequences of 8..128 tokens.  Beside it, as the yardstick, the same encoder written in torch bf16 on the same device
(the ragged batch padded to its longest sequence with an additive key mask, the usual way to batch it there).

One process; the cases and the two implementations are interleaved round by round so that drift hits them alike.  A sample is a
window of back-to-back whole calls (ids as numpy arrays on the host in, embeddings on the host out; every call ends in a device
synchronise) sized from the warm-up to last at least --window seconds; the figure is the window's time per call, reported as the
median over the rounds with the min .. max spread.  The binding's own host work (one np.concatenate of the id arrays) is inside the
window.  No ratio is promised; nothing gates on these figures.

    python tools/embed_throughput.py [--rounds 7] [--window 0.25] [--dtype bf16|f32] [--no-torch]
"""
import argparse
import math
import os
import sys
import time

import numpy as np
import torch  # before the library: torch brings its own HIP runtime, and the first one loaded must be the one both use

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import fastllm_amd as fa  # noqa: E402

CFG = dict(hidden_size=384, num_attention_heads=12, intermediate_size=1536, num_hidden_layers=6, vocab_size=30522,
           max_position_embeddings=512, layer_norm_eps=1e-12)


def shapes(cfg):
    h, i, V, P = cfg["hidden_size"], cfg["intermediate_size"], cfg["vocab_size"], cfg["max_position_embeddings"]
    out = [("embeddings.word_embeddings.weight", (V, h)), ("embeddings.position_embeddings.weight", (P, h)),
           ("embeddings.LayerNorm.weight", (h,)), ("embeddings.LayerNorm.bias", (h,))]
    for l in range(cfg["num_hidden_layers"]):
        p = "encoder.layer.%d." % l
        for nm, s in (("attention.self.query", (h, h)), ("attention.self.key", (h, h)), ("attention.self.value", (h, h)),
                      ("attention.output.dense", (h, h)), ("intermediate.dense", (i, h)), ("output.dense", (h, i))):
            out += [(p + nm + ".weight", s), (p + nm + ".bias", (s[0],))]
        for nm in ("attention.output.LayerNorm", "output.LayerNorm"):
            out += [(p + nm + ".weight", (h,)), (p + nm + ".bias", (h,))]
    return out


def device_weights(cfg):
    g = torch.Generator(device="cuda").manual_seed(9)
    w = {}
    for name, s in shapes(cfg):
        t = torch.randn(s, generator=g, device="cuda", dtype=torch.float32)
        t = 1.0 + 0.1 * t if name.endswith("LayerNorm.weight") else 0.1 * t if name.endswith(".bias") else 0.05 * t
        w[name] = t.to(torch.bfloat16).contiguous()
    torch.cuda.synchronize()
    return w


class TorchEncoder:
    """the same forward in torch bf16: tanh GELU, no token types, eps 1e-12 at the embeddings, padded batch + key mask"""

    def __init__(self, cfg, w):
        self.cfg, self.w = cfg, w

    @torch.no_grad()
    def embed(self, seqs):
        import torch.nn.functional as F
        cfg, w = self.cfg, self.w
        h, H = cfg["hidden_size"], cfg["num_attention_heads"]
        d, B, T = h // H, len(seqs), max(len(s) for s in seqs)
        ids = np.zeros((B, T), np.int64)
        keep = np.zeros((B, T), np.float32)
        for i, s in enumerate(seqs):
            ids[i, :len(s)] = s
            keep[i, :len(s)] = 1.0
        ids, keep = torch.from_numpy(ids).cuda(), torch.from_numpy(keep).cuda()
        bias = ((1.0 - keep) * -1e4).to(torch.bfloat16)[:, None, None, :]
        x = w["embeddings.word_embeddings.weight"][ids] + w["embeddings.position_embeddings.weight"][:T]
        x = F.layer_norm(x, (h,), w["embeddings.LayerNorm.weight"], w["embeddings.LayerNorm.bias"], 1e-12)
        for l in range(cfg["num_hidden_layers"]):
            p = "encoder.layer.%d." % l
            lin = lambda nm, t: F.linear(t, w[p + nm + ".weight"], w[p + nm + ".bias"])      # noqa: E731
            q, k, v = (lin("attention.self." + n, x).view(B, T, H, d).transpose(1, 2) for n in ("query", "key", "value"))
            a = torch.softmax(q @ k.transpose(2, 3) / math.sqrt(d) + bias, dim=-1) @ v
            a = a.transpose(1, 2).reshape(B, T, h)
            x = F.layer_norm(x + lin("attention.output.dense", a), (h,), w[p + "attention.output.LayerNorm.weight"],
                             w[p + "attention.output.LayerNorm.bias"], cfg["layer_norm_eps"])
            f = lin("output.dense", F.gelu(lin("intermediate.dense", x), approximate="tanh"))
            x = F.layer_norm(x + f, (h,), w[p + "output.LayerNorm.weight"], w[p + "output.LayerNorm.bias"], cfg["layer_norm_eps"])
        x = x.float() * keep[:, :, None]
        m = x.sum(1) / keep.sum(1, keepdim=True)
        return (m / m.norm(dim=1, keepdim=True)).cpu().numpy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--window", type=float, default=0.25, help="seconds of back-to-back calls per sample, at least")
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "f32"])
    ap.add_argument("--no-torch", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "no GPU visible"
    w = device_weights(CFG)
    tensors = {k: (t.data_ptr(), fa.binding.BF16, tuple(t.shape), 0) for k, t in w.items()}
    enc = fa.Encoder(CFG, tensors, dtype=a.dtype, max_batch_tokens=32768)
    ref = None if a.no_torch else TorchEncoder(CFG, w)
    rs = np.random.RandomState(1)
    mk = lambda n: rs.randint(0, CFG["vocab_size"], size=n).astype(np.uint32)      # noqa: E731
    cases = [("1 x 16", [mk(16)]), ("1 x 128", [mk(128)]), ("64 x 128", [mk(128) for _ in range(64)]),
             ("256 ragged 8..128", [mk(int(n)) for n in rs.randint(8, 129, size=256)])]
    impls = [("fl_encoder_embed " + a.dtype, enc.embed)] + ([("torch bf16", ref.embed)] if ref else [])
    print("library: %s; shape: all-MiniLM-L6-v2 (h 384, 12 heads, I 1536, 6 layers), random weights" % fa.binding.LIB_PATH)
    def window(f, seqs, reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            f(seqs)                                             # (returns host arrays: the call has synchronised)
        return (time.perf_counter() - t0) / reps * 1e3

    reps = {}
    for name, seqs in cases:                                    # warm-up, the two must agree, and the window sizes
        outs = [f(seqs) for _, f in impls]
        if ref:
            cos = (outs[0] * outs[1]).sum(1)
            print("%-20s cosine library vs torch: min %.6f" % (name, cos.min()))
        for iname, f in impls:
            reps[(name, iname)] = max(3, int(math.ceil(a.window * 1e3 / window(f, seqs, 5))))
    ms = {(c, i): [] for c, _ in cases for i, _ in impls}
    for _ in range(a.rounds):
        for cname, seqs in cases:
            for iname, f in impls:
                ms[(cname, iname)].append(window(f, seqs, reps[(cname, iname)]))
    for cname, seqs in cases:
        for iname, _ in impls:
            v = np.array(ms[(cname, iname)])
            print("%-20s %-24s %8.3f ms per call  (min %.3f .. max %.3f over %d windows of %d calls)  %10.0f sequences/s  %6d tokens"
                  % (cname, iname, np.median(v), v.min(), v.max(), v.size, reps[(cname, iname)], len(seqs) / np.median(v) * 1e3,
                     sum(len(s) for s in seqs)))
    enc.close()


if __name__ == "__main__":
    main()
