"""Speculative decode for full requests without a GPU (the pattern of test_verify_sample_abi.py): fl_forward_verify_lp,
fl_decode_lookup_lp and the two op entry points are exported and declared, and their argument errors -- nulls, n_draft 16, a wrong
fl_logprobs.struct_size, top_n 21, the sampler's -- are decided before the handles are looked at and before the device is probed."""
import ctypes as C
import re
import subprocess

import numpy as np
import pytest

from test_lookup_abi import HEADER
from test_verify_sample_abi import samplers

NEW = ("fl_forward_verify_lp", "fl_decode_lookup_lp", "fl_op_verify_adjust", "fl_op_verify_adjust_time", "fl_op_rules_count")
BAD_ARGUMENT = -8


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


class Lp:
    """an fl_logprobs over live arrays of n rows"""

    def __init__(self, n, top_n=5):
        import fastllm_amd.binding as B
        self.arrays = B._LogprobArrays(n, top_n)
        self.st = self.arrays.struct()
        self.st.top_n = top_n


def logprob_faults():
    """(an fl_logprobs with one fault, the word its message must hold)"""
    size = Lp(17)
    size.st.struct_size -= 8
    top = Lp(17, 20)
    top.st.top_n = 21
    null = Lp(17)
    null.st.token_logprob = None
    return [(size, b"struct_size"), (top, b"top_n"), (null, b"token_logprob")]


def test_verify_argument_errors(L):
    import fastllm_amd.binding as B
    toks = np.zeros(17, np.uint32)
    dr = np.zeros(16, np.uint32)
    n = C.c_size_t(5)
    ok = B.make_sampler(0.8, seed=3, top_p=0.9, top_k=40)
    lp_ok = Lp(17)

    def call(sp, lp, n_draft=3, draft=dr.ctypes.data, tokens=toks.ctypes.data, n_out=C.byref(n)):
        return L.fl_forward_verify_lp(None, None, 1, draft, n_draft, 0, C.byref(sp) if sp is not None else None,
                                      C.byref(lp.st) if lp is not None else None, tokens, n_out, None)

    for sp, word in samplers():
        assert call(sp, lp_ok) == BAD_ARGUMENT and word in L.fl_last_error(), word
    for lp, word in logprob_faults():
        assert call(ok, lp) == BAD_ARGUMENT and word in L.fl_last_error(), word
    assert call(ok, lp_ok, n_draft=16) == BAD_ARGUMENT and b"FL_VERIFY_MAX_DRAFT" in L.fl_last_error()
    assert call(ok, lp_ok, tokens=None) == BAD_ARGUMENT and b"tokens_out" in L.fl_last_error()
    assert call(ok, lp_ok, n_out=None) == BAD_ARGUMENT and b"n_out" in L.fl_last_error()
    assert call(ok, lp_ok, draft=None) == BAD_ARGUMENT and b"draft" in L.fl_last_error()
    for sp in (ok, None, B.make_sampler(0.0)):                               # a well-formed call: only the model is missing
        for lp in (lp_ok, None):
            n.value = 5
            assert call(sp, lp, n_draft=15) == BAD_ARGUMENT and b"null model or cache" in L.fl_last_error() and n.value == 0


def test_loop_argument_errors(L):
    import fastllm_amd.binding as B
    toks = np.zeros(17, np.uint32)
    dr = np.zeros(16, np.uint32)
    n = C.c_size_t(5)
    st = B.FlSpecStats()
    ok = B.make_sampler(0.8, seed=3, top_p=0.9, top_k=40)
    lp_ok = Lp(17)

    def loop(sp, lp, opts=B.make_lookup(), tokens=toks.ctypes.data, n_out=C.byref(n), steps=4):
        return L.fl_decode_lookup_lp(None, None, dr.ctypes.data, 4, 1, 0, steps, -1, C.byref(opts) if opts is not None else None,
                                     C.byref(sp) if sp is not None else None, C.byref(lp.st) if lp is not None else None, tokens, n_out,
                                     C.byref(st))

    for sp, word in samplers():
        assert loop(sp, lp_ok) == BAD_ARGUMENT and word in L.fl_last_error(), word
    for lp, word in logprob_faults():
        assert loop(ok, lp) == BAD_ARGUMENT and word in L.fl_last_error(), word
    assert loop(ok, lp_ok, opts=B.make_lookup(max_draft=16)) == BAD_ARGUMENT and b"max_draft" in L.fl_last_error()
    assert loop(ok, lp_ok, opts=None) == BAD_ARGUMENT
    assert loop(ok, lp_ok, tokens=None) == BAD_ARGUMENT and b"tokens_out" in L.fl_last_error()
    assert loop(ok, lp_ok, n_out=None) == BAD_ARGUMENT and b"n_out" in L.fl_last_error()
    for sp in (ok, None):
        for lp in (lp_ok, None):
            assert loop(sp, lp) == BAD_ARGUMENT and b"null model or cache" in L.fl_last_error()
            assert loop(sp, lp, opts=B.make_lookup(max_draft=0)) == BAD_ARGUMENT and b"null model or cache" in L.fl_last_error()
    assert loop(ok, lp_ok, steps=0) == 0 and n.value == 0                    # nothing to do


def test_op_argument_errors(L):
    import fastllm_amd.binding as B
    V = 8
    lg = np.zeros((2, V), np.float32)
    ids = np.zeros(16, np.uint32)
    w = np.zeros(V, np.uint32)
    b = np.zeros(V, np.float32)
    sc = np.array([1.0, 0.0, 0.0], np.float32)
    out = np.zeros((16, V), np.float32)
    desc, keep = B.make_guide_desc([0, V], np.arange(V, dtype=np.uint32), np.zeros(V, np.uint32))
    states = np.zeros(16, np.uint32)

    def op(T=2, logits=lg.ctypes.data, ids_=ids.ctypes.data, words=w.ctypes.data, biases=b.ctypes.data, scalars=sc.ctypes.data,
           d=C.byref(desc), st=states.ctypes.data, o=out.ctypes.data, v=V):
        return L.fl_op_verify_adjust(logits, T, v, ids_, words, biases, scalars, d, st, o)

    assert op(T=17) == BAD_ARGUMENT and op(T=0) == BAD_ARGUMENT and op(v=0) == BAD_ARGUMENT
    assert op(logits=None) == BAD_ARGUMENT and op(ids_=None) == BAD_ARGUMENT and op(o=None) == BAD_ARGUMENT
    assert op(words=None, d=None) == BAD_ARGUMENT and b"neither" in L.fl_last_error()
    assert op(biases=None) == BAD_ARGUMENT and op(scalars=None) == BAD_ARGUMENT
    assert op(st=None) == BAD_ARGUMENT
    bad = np.ones(16, np.uint32)                                             # state 1 of a one-state automaton
    assert op(st=bad.ctypes.data) == BAD_ARGUMENT and b"n_states" in L.fl_last_error()
    assert op(v=4) == BAD_ARGUMENT                                           # the automaton's ids reach 7
    for kw in (dict(), dict(words=None), dict(d=None)):                      # well-formed: the device, or the loud "no device"
        assert op(**kw) in (0, -9)
    ms = C.c_double(0)
    timed = lambda iters, out: L.fl_op_verify_adjust_time(lg.ctypes.data, 2, V, ids.ctypes.data, w.ctypes.data, b.ctypes.data, sc.ctypes.data, C.byref(desc),
                                                          states.ctypes.data, iters, out)
    assert timed(0, C.byref(ms)) == BAD_ARGUMENT and timed(4, None) == BAD_ARGUMENT and timed(4, C.byref(ms)) in (0, -9)
    del keep
    assert L.fl_op_rules_count(None, V, ids.ctypes.data, 2) == BAD_ARGUMENT
    assert L.fl_op_rules_count(w.ctypes.data, V, None, 2) == BAD_ARGUMENT
    assert L.fl_op_rules_count(w.ctypes.data, V, ids.ctypes.data, 17) == BAD_ARGUMENT
    assert L.fl_op_rules_count(w.ctypes.data, 0, ids.ctypes.data, 2) == BAD_ARGUMENT
    assert L.fl_op_rules_count(w.ctypes.data, V, ids.ctypes.data, 2) in (0, -9)


class Recorder:
    """stands in for the loaded library: records which entry point a Model method calls"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def f(*a):
            self.calls.append(name)
            return 0
        return f


def test_python_methods_reach_the_new_entry_points(monkeypatch):
    import fastllm_amd.binding as B
    rec = Recorder()
    monkeypatch.setattr(B, "lib", lambda: rec)
    m = B.Model.__new__(B.Model)
    m._h, m.V = None, 8
    c = B.Cache.__new__(B.Cache)
    c._h = None
    toks, lg = m.forward_verify_lp(c, 1, [2, 3], 0)
    assert lg is None and len(toks) == 0
    assert len(m.forward_verify_lp(c, 1, [2, 3], 0, logprobs=5, temperature=0.8, want_logits=True)) == 5
    m.decode_lookup_lp(c, [1, 2, 3], 1, 0, 4)
    assert len(m.decode_lookup_lp(c, [1, 2, 3], 1, 0, 4, logprobs=0, temperature=0.8, top_p=0.9, draws_done=1, return_stats=True)) == 5
    assert rec.calls == ["fl_forward_verify_lp"] * 2 + ["fl_decode_lookup_lp"] * 2
    m.forward_verify(c, 1, [2, 3], 0)                                        # the old methods keep their entry points
    m.decode_lookup(c, [1, 2, 3], 1, 0, 4)
    assert rec.calls[4:] == ["fl_forward_verify", "fl_decode_lookup"]
