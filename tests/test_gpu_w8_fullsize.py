"""The FP8 decode mode at full size: Mistral-7B shapes, full depth, synthetic weights generated in HBM with torch (as bench.py does)."""
import os
import sys

import numpy as np
import pytest

import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# torch brings its own copy of the HIP runtime, which only sees the GPU if it initialises BEFORE the product library's does (the order
# bench.py has; tests/conftest.py): let it go first when this module is collected
try:
    import torch
    torch.cuda.is_available()
except Exception:                                          # (a machine without torch / without a GPU: the test below is a gpu test)
    torch = None


def test_fp8_mistral_7b_full_depth():
    """Mistral-7B shapes at full depth, synthetic weights generated in HBM: 16-token prompt + 8 decode steps.  Rule 4 (the prompt's
    logits equal the bf16 model's on the image, bit for bit) and rule 1 with the bf16 model on W' as the truth's stand-in: no CPU
    oracle runs 7B in test time, so e_x here is measured against the fp32-compute GPU model on W' (tests/test_gpu_fullsize_7b.py
    holds that model to the oracle at full width)."""
    import fastllm_amd as fa
    sys.path.insert(0, ROOT)
    import bench
    from fastllm_amd.configs import MODEL_CONFIGS
    from test_w8_abi import PROJECTIONS
    assert torch.cuda.is_available()
    cfg = MODEL_CONFIGS["mistral-7b"]
    dev = torch.device("cuda", 0)
    wts = bench.synth_device_weights(torch, cfg, dev, seed=21)
    g8 = fa.Model(cfg, bench.as_fl_tensors(wts, 0), dtype="bf16", decode_weights="e4m3")
    # W' on the device with torch: the same definition as the restatement (frexp scale, float8_e4m3fn RNE)
    for name in list(wts):
        if name.endswith(PROJECTIONS):
            t = wts[name].float()
            amax = t.abs().amax(dim=1)
            m, x = torch.frexp(amax)
            e = torch.where(m <= 0.875, x - 9, x - 8)
            e = torch.where(amax == 0, torch.zeros_like(e), e.clamp(min=-126))
            s = torch.ldexp(torch.ones_like(amax), e)
            q = (t / s[:, None]).to(torch.float8_e4m3fn)
            wts[name] = (q.float() * s[:, None]).to(torch.bfloat16)
            assert torch.equal(wts[name].float(), q.float() * s[:, None])
            del t, q
    torch.cuda.synchronize()
    tens = bench.as_fl_tensors(wts, 0)
    g16 = fa.Model(cfg, tens, dtype="bf16")
    ids = synth.prompt_ids(cfg, 16, seed=2)
    forced = synth.prompt_ids(cfg, 8, seed=4)
    out = {}
    for k, m in (("g8", g8), ("g16", g16)):
        c = m.new_cache(64)
        lg = [m.forward(c, ids, 0)]
        for i in range(8):
            lg.append(m.forward(c, forced[i:i + 1], 16 + i))
        out[k] = np.stack(lg)
        c.close()
    g8.close(); g16.close()
    assert np.array_equal(out["g8"][0], out["g16"][0])                        # rule 4
    g32 = fa.Model(cfg, tens, dtype="f32")
    c = g32.new_cache(64)
    lg = [g32.forward(c, ids, 0)]
    for i in range(8):
        lg.append(g32.forward(c, forced[i:i + 1], 16 + i))
    ref = np.stack(lg)
    g32.close()
    n = np.linalg.norm(ref)
    e_g8, e_g16 = np.linalg.norm(out["g8"] - ref) / n, np.linalg.norm(out["g16"] - ref) / n
    print("\nmistral-7b full depth: rel L2 to fp32 on W' -- fp8 decode %.3e, bf16 %.3e; fp8 vs bf16 %.3e" % (e_g8, e_g16, np.linalg.norm(out["g8"] - out["g16"]) / n))
    assert e_g8 <= 1.5 * e_g16 + 1e-4, (e_g8, e_g16)                          # rule 1
