"""Per-draw cost of the device token selection by mode: ArgMax, Sampling::All, top-p 0.9 on random logits, and the worst case for
the band walk (flat logits, top_p 0.999), at V = 32000 and V = 152064.

One process; the modes are interleaved round by round so that drift hits them alike; every figure is one call of many draws
(launch included), reported as the median over the rounds with the min .. max spread.  A library without fl_op_sample_ex (FL_LIB_PATH
pointing at an older build) reports the first two modes only -- that is how the parent commit's figures are taken.

    python tools/sample_cost_modes.py [--draws 1000] [--rounds 7]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import fastllm_amd as fa  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--draws", type=int, default=1000)
    ap.add_argument("--rounds", type=int, default=7)
    a = ap.parse_args()
    has_ex = hasattr(fa.lib(), "fl_op_sample_ex")
    print("library: %s (fl_op_sample_ex: %s)" % (fa.binding.LIB_PATH, "yes" if has_ex else "no"))
    for V in (32000, 152064):
        rnd = (np.random.RandomState(0).randn(V) * 2.5).astype(np.float32)
        flat = np.zeros(V, np.float32)
        modes = [("ArgMax", rnd, dict(temperature=0.0)), ("Sampling::All", rnd, dict(temperature=1.0))]
        if has_ex:
            modes += [("top-p 0.9, random logits", rnd, dict(temperature=1.0, top_p=0.9)),
                      ("top-k 40, random logits", rnd, dict(temperature=1.0, top_k=40)),
                      ("top-p 0.999, flat logits (worst case)", flat, dict(temperature=1.0, top_p=0.999))]
        for _, lg, kw in modes:
            fa.op_sample(lg, 5, **kw)
        us = {name: [] for name, _, _ in modes}
        for _ in range(a.rounds):
            for name, lg, kw in modes:
                n = a.draws if "worst" not in name else max(20, a.draws // 20)
                t0 = time.perf_counter()
                fa.op_sample(lg, n, **kw)
                us[name].append((time.perf_counter() - t0) / n * 1e6)
        for name, _, _ in modes:
            v = np.array(us[name])
            print("V=%6d  %-40s %9.1f us per draw  (min %.1f .. max %.1f over %d rounds)" % (V, name, np.median(v), v.min(), v.max(), v.size))


if __name__ == "__main__":
    main()
