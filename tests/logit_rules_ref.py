"""The logit rules (fl_cache_set_logit_rules) restated in numpy float32: the yardstick of the logit-rules tests.  Every operation is
a float32 operation of its own, in the order the header states, so the device result is compared bit for bit.

    y = x[j]
    if word != 0 and rp != 1:  y = y / rp if y > 0 else y * rp
    if c > 0:                  y = y - float32(c) * fp;  y = y - pp          (c = word & 0x7fffffff)
    y = y + bias
"""
import numpy as np

PROMPT_BIT = np.uint32(0x80000000)
COUNT_MASK = np.uint32(0x7FFFFFFF)


def table(V, prompt_ids=(), output_ids=(), logit_bias=None):
    """The table an install builds: words uint32 [V] (bit 31: in the prompt, bits 0..30: times produced) and biases float32 [V]."""
    words = np.zeros(V, np.uint32)
    words[np.asarray(list(prompt_ids), dtype=np.int64)] |= PROMPT_BIT
    for t in output_ids:
        words[int(t)] += np.uint32(1)
    bias = np.zeros(V, np.float32)
    for j, v in (logit_bias.items() if hasattr(logit_bias, "items") else (logit_bias or ())):
        bias[int(j)] = np.float32(v)
    return words, bias


def count(words, token):
    """One more output of `token` (in place); an id the table does not have counts nothing, and a count of 2^31 - 1 stays."""
    if 0 <= int(token) < words.size and (words[int(token)] & COUNT_MASK) != COUNT_MASK:
        words[int(token)] += np.uint32(1)
    return words


def apply(x, words, bias, rp=1.0, fp=0.0, pp=0.0):
    """The adjusted row, float32 [V]."""
    x = np.asarray(x, dtype=np.float32)
    words = np.asarray(words, dtype=np.uint32)
    bias = np.asarray(bias, dtype=np.float32)
    rp, fp, pp = np.float32(rp), np.float32(fp), np.float32(pp)
    with np.errstate(all="ignore"):
        y = x.copy()
        if rp != np.float32(1.0):
            seen = words != 0
            y = np.where(seen, np.where(y > 0, y / rp, y * rp), y).astype(np.float32)
        c = words & COUNT_MASK
        cf = c.astype(np.float32)
        y = np.where(c > 0, ((y - cf * fp).astype(np.float32) - pp).astype(np.float32), y).astype(np.float32)
        y = (y + bias).astype(np.float32)
    return y


def argmax_last(y):
    """ArgMax as the device takes it: the LAST maximal index."""
    return int(np.flatnonzero(y == y.max())[-1])


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
