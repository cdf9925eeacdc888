"""Speculative decode for sampled requests without a GPU: the new entry points (the two calls, the kernel alone and its timed form) are
exported and declared, their argument errors are decided before the handles are looked at (the pattern of test_lookup_abi.py), and the
Python keyword defaults still reach the greedy entry points."""
import ctypes as C
import re
import subprocess

import numpy as np
import pytest

from test_lookup_abi import HEADER

NEW = ("fl_forward_verify_ex", "fl_decode_lookup_ex", "fl_op_verify_sample", "fl_op_verify_sample_time")


@pytest.fixture(scope="module")
def L():
    import fastllm_amd
    return fastllm_amd.lib()


def test_new_symbols_are_exported_and_declared(L):
    hdr = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name in NEW:
        assert hasattr(L, name), name
        assert re.search(r"\b%s\s*\(" % name, hdr), name
    out = subprocess.check_output(["nm", "-D", "--defined-only", __import__("fastllm_amd").binding.LIB_PATH], text=True)
    assert set(NEW) <= set(re.findall(r" T (fl_[a-z_0-9]+)", out))
    assert L.fl_abi_version() == 2                                           # the change only adds entries


def samplers():
    """(a sampler with one fault, the word its message must hold)"""
    import fastllm_amd.binding as B
    size = B.make_sampler(0.8)
    size.struct_size -= 8
    return [(size, b"struct_size"), (B.make_sampler(0.8, top_p=float("nan")), b"NaN"), (B.make_sampler(0.8, top_k=-1), b"top_k")]


def test_verify_argument_errors(L):
    import fastllm_amd.binding as B
    toks = np.zeros(17, np.uint32)
    dr = np.zeros(16, np.uint32)
    n = C.c_size_t(5)
    ok = B.make_sampler(0.8, seed=3, top_p=0.9, top_k=40)

    def call(sp, n_draft=3, draft=dr.ctypes.data, tokens=toks.ctypes.data, n_out=C.byref(n)):
        return L.fl_forward_verify_ex(None, None, 1, draft, n_draft, 0, C.byref(sp) if sp is not None else None, tokens, n_out, None)

    for sp, word in samplers():
        assert call(sp) == -8 and word in L.fl_last_error(), word
    assert call(ok, n_draft=16) == -8 and b"FL_VERIFY_MAX_DRAFT" in L.fl_last_error()
    assert call(ok, tokens=None) == -8 and b"tokens_out" in L.fl_last_error()
    assert call(ok, n_out=None) == -8 and b"n_out" in L.fl_last_error()
    assert call(ok, draft=None) == -8 and b"draft" in L.fl_last_error()
    for sp in (ok, None, B.make_sampler(0.0)):                               # a well-formed call: only the model is missing
        n.value = 5
        assert call(sp, n_draft=15) == -8 and b"null model or cache" in L.fl_last_error() and n.value == 0


def test_loop_argument_errors(L):
    import fastllm_amd.binding as B
    toks = np.zeros(17, np.uint32)
    dr = np.zeros(16, np.uint32)
    n = C.c_size_t(5)
    st = B.FlSpecStats()
    ok = B.make_sampler(0.8, seed=3, top_p=0.9, top_k=40)

    def loop(sp, opts=B.make_lookup(), tokens=toks.ctypes.data, n_out=C.byref(n), steps=4):
        return L.fl_decode_lookup_ex(None, None, dr.ctypes.data, 4, 1, 0, steps, -1, C.byref(opts) if opts is not None else None,
                                     C.byref(sp) if sp is not None else None, tokens, n_out, C.byref(st))

    for sp, word in samplers():
        assert loop(sp) == -8 and word in L.fl_last_error(), word
    assert loop(ok, opts=B.make_lookup(max_draft=16)) == -8 and b"max_draft" in L.fl_last_error()
    assert loop(ok, opts=None) == -8
    assert loop(ok, tokens=None) == -8 and b"tokens_out" in L.fl_last_error()
    assert loop(ok, n_out=None) == -8 and b"n_out" in L.fl_last_error()
    for sp in (ok, None):
        assert loop(sp) == -8 and b"null model or cache" in L.fl_last_error()
        assert loop(sp, opts=B.make_lookup(max_draft=0)) == -8 and b"null model or cache" in L.fl_last_error()
    assert loop(ok, steps=0) == 0 and n.value == 0                           # nothing to do


def test_op_argument_errors(L):
    import fastllm_amd.binding as B
    lg = np.zeros((2, 8), np.float32)
    toks = np.zeros(17, np.uint32)
    dr = np.zeros(16, np.uint32)
    acc = C.c_int64(0)
    ok = B.make_sampler(0.8)

    def op(sp, T=2, logits=lg.ctypes.data, draft=dr.ctypes.data, tokens=toks.ctypes.data, n_acc=C.byref(acc)):
        return L.fl_op_verify_sample(logits, T, 8, draft, C.byref(sp) if sp is not None else None, tokens, n_acc, None)

    assert op(ok, T=17) == -8 and op(ok, T=0) == -8
    assert op(ok, draft=None) == -8 and op(ok, logits=None) == -8 and op(ok, tokens=None) == -8 and op(ok, n_acc=None) == -8
    assert op(None) == -8
    for sp, word in samplers():
        assert op(sp) == -8 and word in L.fl_last_error(), word
    assert op(B.make_sampler(0.0)) == -8 and b"ArgMax" in L.fl_last_error()  # the greedy selection is fl_op_verify_select
    assert op(ok) in (0, -9)                                                 # a well-formed call reaches the device or the loud "no device"
    # the timed form (tools/verify_sample_cost.py)
    ms = (C.c_double * 2)()
    it = (C.c_int32 * 2)(1, 1)
    assert L.fl_op_verify_sample_time(lg.ctypes.data, 17, 8, C.byref(ok), it, ms) == -8
    assert L.fl_op_verify_sample_time(lg.ctypes.data, 2, 8, C.byref(ok), None, ms) == -8
    assert L.fl_op_verify_sample_time(lg.ctypes.data, 2, 8, C.byref(ok), (C.c_int32 * 2)(-1, 1), ms) == -8
    assert L.fl_op_verify_sample_time(lg.ctypes.data, 2, 8, C.byref(B.make_sampler(0.0)), it, ms) == -8
    assert L.fl_op_verify_sample_time(lg.ctypes.data, 2, 8, C.byref(ok), it, ms) in (0, -9)


class Recorder:
    """stands in for the loaded library: records which entry point a Model method calls"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def f(*a):
            self.calls.append(name)
            return 0
        return f


def test_python_defaults_reach_the_greedy_entry_points(monkeypatch):
    import fastllm_amd.binding as B
    rec = Recorder()
    monkeypatch.setattr(B, "lib", lambda: rec)
    m = B.Model.__new__(B.Model)
    m._h, m.V = None, 8
    c = B.Cache.__new__(B.Cache)
    c._h = None
    m.forward_verify(c, 1, [2, 3], 0)
    m.decode_lookup(c, [1, 2, 3], 1, 0, 4)
    assert rec.calls == ["fl_forward_verify", "fl_decode_lookup"]
    m.forward_verify(c, 1, [2, 3], 0, temperature=0.8)
    m.decode_lookup(c, [1, 2, 3], 1, 0, 4, temperature=0.8, top_p=0.9, draws_done=1)
    assert rec.calls[2:] == ["fl_forward_verify_ex", "fl_decode_lookup_ex"]
