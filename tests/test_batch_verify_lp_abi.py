"""fl_batch_verify_lp / fl_batch_decode_lookup_lp / fl_op_verify_adjust_packed without a GPU: declared in the header, exported by the
library, and their argument errors precede the device probe (FL_ERR_BAD_ARGUMENT, never FL_ERR_NO_DEVICE)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import fastllm_amd as fa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["fl_batch_verify_lp", "fl_batch_decode_lookup_lp", "fl_op_verify_adjust_packed"]
BAD_ARGUMENT = -8


@pytest.mark.parametrize("name", NAMES)
def test_declared_and_exported(name):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fastllm_mi355x.h")).read(), flags=re.S)
    assert re.search(r"\bint %s\s*\(" % name, hdr)
    assert getattr(fa.lib(), name) is not None


def test_argument_errors_precede_the_device_probe():
    L = fa.lib()
    one = (C.c_void_p * 1)(None)
    ids, off, pos = np.zeros(2, np.uint32), np.array([0, 2], np.uint64), np.zeros(1, np.uint64)
    toks, n_out = np.zeros(2, np.uint32), np.array([7], np.uint64)
    p = lambda a: a.ctypes.data
    assert L.fl_batch_verify_lp(None, C.cast(one, C.c_void_p), 0, p(ids), p(off), p(pos), None, None, p(toks), p(n_out), None) == BAD_ARGUMENT
    assert L.fl_batch_verify_lp(None, C.cast(one, C.c_void_p), 1, p(ids), p(off), p(pos), None, None, None, p(n_out), None) == BAD_ARGUMENT
    assert n_out[0] == 0
    n_out[0] = 7
    assert L.fl_batch_verify_lp(None, C.cast(one, C.c_void_p), 1, p(ids), p(off), p(pos), None, None, p(toks), p(n_out), None) == BAD_ARGUMENT
    assert n_out[0] == 0
    lp = (fa.binding.FlLogprobs * 1)()
    lp[0].top_n = 0
    assert L.fl_batch_verify_lp(None, C.cast(one, C.c_void_p), 1, p(ids), p(off), p(pos), None, C.cast(lp, C.c_void_p), p(toks), p(n_out), None) == BAD_ARGUMENT
    assert b"struct_size" in L.fl_last_error()
    steps = np.array([4], np.uint64)
    assert L.fl_batch_decode_lookup_lp(None, C.cast(one, C.c_void_p), 1, None, p(off), p(ids), p(pos), p(steps), None, None, None,
                                       C.cast(lp, C.c_void_p), p(toks), p(n_out), None) == BAD_ARGUMENT
    x = np.zeros((17, 4), np.float32)
    with pytest.raises(fa.FastLLMError) as e:
        fa.op_verify_adjust_packed(x, [0, 17], np.zeros(17, np.uint32), words=np.zeros((1, 4), np.uint32), biases=np.zeros((1, 4)), scalars=[[1, 0, 0]])
    assert e.value.code == BAD_ARGUMENT
