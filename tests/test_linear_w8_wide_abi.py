"""fl_op_linear_w8_wide / fl_op_linear_w8_wide_plan without a GPU: argument errors and refusals precede the device probe; the
planner's slices."""
import numpy as np

import fastllm_amd as fa

BAD_ARGUMENT, UNSUPPORTED = -8, -10


def test_argument_errors_refusals_and_plan_need_no_device():
    x, q, s = np.zeros((17, 64), np.uint16), np.zeros((4, 64), np.uint8), np.ones(4, np.float32)
    y = np.full((17, 4), 7.0, np.float32)
    p = lambda a: a.ctypes.data if a is not None else None

    def rc(x=x, q=q, s=s, T=17, N=4, K=64, epi=0, y=y):
        return fa.lib().fl_op_linear_w8_wide(p(x), p(q), p(s), None, T, N, K, epi, 0, None, p(y))

    assert rc(x=None) == rc(q=None) == rc(s=None) == rc(y=None) == BAD_ARGUMENT and b"null" in fa.lib().fl_last_error()
    assert rc(N=0) == rc(epi=2) == rc(epi=1, N=3) == BAD_ARGUMENT
    assert rc(T=16) == rc(T=65) == rc(K=72) == UNSUPPORTED and b"17..64 rows" in fa.lib().fl_last_error()
    assert (y == 7.0).all()
    plan = fa.op_linear_w8_wide_plan
    assert plan(16, 64, 64) == plan(65, 64, 64) == plan(17, 64, 72) == plan(17, 64, 64, epilogue=2) == 0
    assert plan(17, 1, 16) == plan(64, 64, 64) == 1 and plan(64, 4096, 14336) > 1      # few row groups, a long K: slices ...
    assert plan(64, 28672, 14336, epilogue=1) == 1                                    # ... which gate/up never takes
    assert fa.op_linear_w8_plan(17, 64, 64) == 0                                      # (the 16-row kernel's plan is what it was)

