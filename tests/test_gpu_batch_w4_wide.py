"""A decode batch of 17-64 members of an MXFP4 model under fl_tune "rows_w4" reads the e2m1 nibbles through k_gemm_rows64_w4.hip, in
the shape of tests/test_gpu_rows_w4_model.py::test_batch_step_streams_the_nibbles: switch 0 is the bf16 model of W' bit for bit,
switch 1 differs in fp32 summation order only."""
import numpy as np
import pytest

from test_gpu_batch_w8 import members, oracle_row, rel
from test_gpu_rows_w4_model import models, w4_launches

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fa():
    import fastllm_amd
    assert fastllm_amd.device_count() >= 1
    return fastllm_amd


@pytest.mark.parametrize("B", [17, 64])
def test_wide_batch_step_streams_the_nibbles(fa, B):
    cfg, g4, g16, om = models(fa, "mistral_a")

    def step(m, switch):
        fa.tune("rows_w4", switch)
        caches, toks, pos = members(m, cfg, range(B))
        b = fa.Batch(m, caches)                                             # (created after the tune call: the switch is read there)
        (lg, _), n_w4 = w4_launches(m, lambda: b.forward(toks, pos, want_logits=True))
        assert [len(c) for c in caches] == [p + 1 for p in pos]
        return lg, toks, n_w4

    try:
        (on, toks, n_on), (off, toks_off, n_off), (ref16, toks16, _) = step(g4, 1), step(g4, 0), step(g16, 1)
    finally:
        fa.tune("rows_w4", 0)
    assert toks == toks_off == toks16
    ref = np.stack([oracle_row(om, cfg, i, t) for i, t in enumerate(toks)])
    assert np.array_equal(off, ref16) and n_off == 0
    assert not np.array_equal(on, off) and n_on > 0
    e4, e16 = rel(on, ref), rel(ref16, ref)
    print("\nB %d: rel L2 to fp32 on W' -- mxfp4 batch %.3e, bf16 %.3e, %d w4 launches" % (B, e4, e16, n_on))
    assert e4 <= 1.5 * e16 + 1e-4, (e4, e16)
    g4.close(); g16.close()
