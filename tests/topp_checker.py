"""numpy restatement of candle's Sampling::TopP / TopK / TopKThenTopP [UPSTREAM-RECALLED], built on the oracle's Sampling::All:
the checker of the device's and the host mirror's nucleus / top-k token selection (tests only).

prs comes from oracle.orc_sample's scratch buffer (softmax(logits / temperature), left-to-right fp32 denominator); the kept prefix
is cut by a sequential fp32 cumulative sum over the stable descending order; the draw is the oracle's multinomial (left-to-right
fp32 cumulative weights, UniformFloat scale loop, one ChaCha12 word, partition_point) over the masked vector in vocabulary order.
"""
import ctypes as C

import numpy as np

from oracle import oracle

MARGIN = 1e-6          # |chosen - boundary| below which a 1-ulp difference in an exp may flip the token (tests/test_gpu_sampler.py)
F32 = np.float32


def prs_of(logits, temperature):
    """softmax(logits / temperature) as the oracle's Sampling::All computes it: a throwaway sampler, a scratch buffer of our own."""
    a = np.ascontiguousarray(logits, dtype=np.float32)
    scratch = np.empty_like(a)
    s = oracle.Sampler(0, temperature)
    oracle.lib().orc_sample(C.byref(s._s), a.ctypes.data, a.size, scratch.ctypes.data, None)
    return scratch


def kept_prefix(prs, top_p=None, top_k=None):
    """(order, m, margin): the stable descending order, the length of the kept prefix, and the distance of top_p from the nearest
    sequential cumulative sum (None without top-p)."""
    V = prs.size
    order = np.argsort(-prs, kind="stable")
    m, margin = V, None
    if top_p is not None and 0.0 < top_p < 1.0:
        c = np.cumsum(prs[order], dtype=np.float32)
        m = min(V, 1 + int(np.count_nonzero(c < F32(top_p))))
        margin = float(np.abs(c.astype(np.float64) - float(F32(top_p))).min())
    if top_k is not None and 0 < top_k < V:
        m = min(m, int(top_k))
    return order, m, margin


class Checker:
    """LogitsProcessor::from_sampling(seed, TopP / TopK / TopKThenTopP / All) on fixed probabilities `prs`."""

    def __init__(self, prs, top_p=None, top_k=None):
        self.V = prs.size
        self.order, self.m, self.margin = kept_prefix(prs, top_p, top_k)
        masked = np.zeros_like(prs)
        keep = self.order[: self.m]
        masked[keep] = prs[keep]
        self.cum = np.cumsum(masked, dtype=np.float32)
        total = self.cum[-1]
        scale = total
        while F32(scale * F32(1.0 - 1.1920929e-07)) >= total:
            scale = np.nextafter(scale, F32(0.0))
        self.scale = F32(scale)

    def draw(self, u):
        """token and the distance of `chosen` from the nearer end of the token's cumulative interval"""
        v12 = np.array([(u >> 9) | 0x3F800000], dtype=np.uint32).view(np.float32)[0]
        chosen = F32(F32(v12 - F32(1.0)) * self.scale)
        tok = int(np.count_nonzero(self.cum[: self.V - 1] <= chosen))
        lo = float(self.cum[tok - 1]) if tok > 0 else 0.0
        return tok, min(abs(float(chosen) - lo), abs(float(chosen) - float(self.cum[tok])))


def compare_draws(got, chk, seed, draws_done=0):
    """tokens `got` against the checker driven by the oracle's ChaCha12 stream: the number of draws that differ, each of which must
    sit within MARGIN of a boundary"""
    o = oracle.Sampler(seed, 1.0)
    for _ in range(draws_done):
        o.next_u32()
    n_diff = 0
    for i, g in enumerate(got):
        tok, near = chk.draw(o.next_u32())
        if int(g) != tok:
            n_diff += 1
            assert near <= MARGIN, "draw %d: got %d, checker %d, %.3g from a boundary" % (i, int(g), tok, near)
    return n_diff
