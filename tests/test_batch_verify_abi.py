"""Packed verify without a GPU: the three new entry points (fl_batch_verify, fl_batch_decode_lookup, the kernel alone) are exported and
declared, every argument error that needs neither a model nor a device is decided before either is looked at -- the calls below pass a
null model -- and names its field, and n_out is zeroed on error (the pattern of test_verify_sample_abi.py)."""
import ctypes as C
import re
import subprocess

import numpy as np
import pytest

from test_lookup_abi import HEADER

NEW = ("fl_batch_verify", "fl_batch_decode_lookup", "fl_op_verify_packed")


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


def bad_samplers(n, at):
    """(an array of n samplers whose entry `at` has one fault, the word its message must hold)"""
    import fastllm_amd.binding as B
    out = []
    for make, word in ((lambda: B.make_sampler(0.8), b"struct_size"), (lambda: B.make_sampler(0.8, top_p=float("nan")), b"NaN"),
                       (lambda: B.make_sampler(0.8, top_k=-1), b"top_k")):
        arr = (B.FlSampler * n)(*[B.make_sampler(0.8, seed=i) for i in range(n)])
        arr[at] = make()
        if word == b"struct_size":
            arr[at].struct_size -= 8
        out.append((arr, word))
    return out


def good_samplers(n):
    import fastllm_amd.binding as B
    return (B.FlSampler * n)(*[B.make_sampler(0.8 if i % 2 else 0.0, seed=i, top_p=0.9, top_k=40) for i in range(n)])


def test_verify_argument_errors(L):
    n = 3
    caches = (C.c_void_p * n)(0x1000, 0x2000, 0x3000)                        # never dereferenced: the model is null
    ids = np.zeros(64, np.uint32)
    offs = np.array([0, 1, 9, 25], np.uint64)
    pos = np.zeros(n, np.uint64)
    toks = np.zeros(64, np.uint32)
    nout = np.full(n, 5, np.uint64)

    def call(n_=n, caches_=caches, ids_=ids.ctypes.data, offs_=offs, pos_=pos.ctypes.data, sp=None, toks_=toks.ctypes.data, nout_=nout):
        nout[:] = 5
        return L.fl_batch_verify(None, C.cast(caches_, C.c_void_p) if caches_ is not None else None, n_, ids_,
                                 offs_.ctypes.data if offs_ is not None else None, pos_, C.cast(sp, C.c_void_p) if sp is not None else None,
                                 toks_, nout_.ctypes.data if nout_ is not None else None, None)

    def refused(word, **kw):
        assert call(**kw) == -8 and word in L.fl_last_error(), (word, L.fl_last_error())
        if kw.get("nout_", nout) is not None and 1 <= kw.get("n_", n) <= 64:
            assert (nout[: kw.get("n_", n)] == 0).all(), word               # zeroed on error

    refused(b"1..64", n_=0)
    refused(b"1..64", n_=65)
    refused(b"null caches, ids, offsets or pos", caches_=None)
    refused(b"null caches, ids, offsets or pos", ids_=None)
    refused(b"null caches, ids, offsets or pos", offs_=None)
    refused(b"null caches, ids, offsets or pos", pos_=None)
    refused(b"tokens_out", toks_=None)
    refused(b"n_out", nout_=None)
    for at in (0, 2):
        for sp, word in bad_samplers(n, at):
            refused(word, sp=sp)
    refused(b"offsets[0]", offs_=np.array([1, 2, 9, 25], np.uint64))
    refused(b"sequence 1 is empty", offs_=np.array([0, 4, 4, 9], np.uint64))
    refused(b"sequence 2 is empty", offs_=np.array([0, 4, 9, 8], np.uint64))
    refused(b"FL_VERIFY_MAX_DRAFT", offs_=np.array([0, 1, 18, 25], np.uint64))      # a 17-row member
    refused(b"cache 2 appears twice", caches_=(C.c_void_p * n)(0x1000, 0x2000, 0x1000))
    refused(b"cache 1 is null", caches_=(C.c_void_p * n)(0x1000, 0, 0x3000))
    # a well-formed call (16-row members included): only the model is missing
    for sp in (None, good_samplers(n)):
        refused(b"null model", sp=sp)


def test_loop_argument_errors(L):
    import fastllm_amd.binding as B
    n = 2
    caches = (C.c_void_p * n)(0x1000, 0x2000)
    corpus = np.zeros(8, np.uint32)
    coff = np.array([0, 3, 8], np.uint64)
    first = np.zeros(n, np.uint32)
    pos = np.zeros(n, np.uint64)
    steps = np.array([4, 6], np.uint64)
    eos = np.array([-1, 3], np.int64)
    toks = np.zeros((n, 6), np.uint32)
    nout = np.full(n, 5, np.uint64)
    st = (B.FlSpecStats * n)()

    def loop(n_=n, caches_=caches, corpus_=corpus.ctypes.data, coff_=coff, first_=first.ctypes.data, pos_=pos.ctypes.data, steps_=steps,
             opts=B.make_lookup(), sp=None, toks_=toks.ctypes.data, nout_=nout):
        nout[:] = 5
        return L.fl_batch_decode_lookup(None, C.cast(caches_, C.c_void_p) if caches_ is not None else None, n_, corpus_,
                                        coff_.ctypes.data if coff_ is not None else None, first_, pos_,
                                        steps_.ctypes.data if steps_ is not None else None, eos.ctypes.data,
                                        C.byref(opts) if opts is not None else None, C.cast(sp, C.c_void_p) if sp is not None else None,
                                        toks_, nout_.ctypes.data if nout_ is not None else None, C.cast(st, C.c_void_p))

    def refused(word, **kw):
        assert loop(**kw) == -8 and word in L.fl_last_error(), (word, L.fl_last_error())
        if kw.get("nout_", nout) is not None and 1 <= kw.get("n_", n) <= 64:
            assert (nout[: kw.get("n_", n)] == 0).all(), word

    refused(b"1..64", n_=0)
    refused(b"1..64", n_=65)
    refused(b"max_draft", opts=B.make_lookup(max_draft=16))
    refused(b"fl_lookup", opts=None)
    for sp, word in bad_samplers(n, 1):
        refused(word, sp=sp)
    refused(b"n_out", nout_=None)
    for k in ("caches_", "coff_", "first_", "pos_", "steps_"):
        refused(b"null caches, corpus_offsets, first_tokens, pos or n_steps", **{k: None})
    refused(b"corpus_offsets decrease", coff_=np.array([0, 5, 3], np.uint64))
    refused(b"null corpus", corpus_=None)
    refused(b"tokens_out", toks_=None)
    for sp in (None, good_samplers(n)):
        refused(b"null model", sp=sp)
        refused(b"null model", sp=sp, opts=B.make_lookup(max_draft=0))
    assert loop(steps_=np.zeros(n, np.uint64)) == 0 and (nout == 0).all()    # nothing to do


def test_op_argument_errors(L):
    lg = np.zeros((6, 8), np.float32)
    ids = np.zeros(6, np.uint32)
    offs = np.array([0, 2, 6], np.uint64)
    toks = np.zeros(6, np.uint32)
    acc = np.zeros(2, np.int64)

    def op(T=6, V=8, n_seq=2, logits=lg.ctypes.data, offs_=offs, ids_=ids, sp=None, block=0, toks_=toks.ctypes.data, acc_=acc.ctypes.data, iters=0):
        return L.fl_op_verify_packed(logits, T, V, n_seq, offs_.ctypes.data if offs_ is not None else None,
                                     ids_.ctypes.data if ids_ is not None else None, C.cast(sp, C.c_void_p) if sp is not None else None, block,
                                     toks_, acc_, None, iters, None)

    for kw in (dict(logits=None), dict(offs_=None), dict(ids_=None), dict(toks_=None), dict(acc_=None)):
        assert op(**kw) == -8 and b"null argument" in L.fl_last_error()
    assert op(T=0) == -8 and op(T=1025) == -8 and b"1 <= T <= 1024" in L.fl_last_error()
    assert op(n_seq=0) == -8 and op(n_seq=65) == -8 and b"n_seq" in L.fl_last_error()
    assert op(block=-1) == -8 and op(iters=-1) == -8
    assert op(offs_=np.array([0, 2, 5], np.uint64)) == -8 and b"offsets" in L.fl_last_error()
    assert op(offs_=np.array([0, 0, 6], np.uint64)) == -8 and b"member 0" in L.fl_last_error()
    big = np.zeros((20, 8), np.float32)
    assert op(T=20, logits=big.ctypes.data, ids_=np.zeros(20, np.uint32), offs_=np.array([0, 17, 20], np.uint64)) == -8
    assert b"1..16 rows" in L.fl_last_error()                                # a 17-row member
    assert op(ids_=np.array([0, 0, 0, 8, 0, 0], np.uint32)) == -8 and b"ids[3]" in L.fl_last_error()
    for sp, word in bad_samplers(2, 1):
        assert op(sp=sp) == -8 and word in L.fl_last_error(), word
    for sp in (None, good_samplers(2)):
        assert op(sp=sp) in (0, -9)                                          # a well-formed call reaches the device or the loud "no device"


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
    cs = []
    for _ in range(2):
        c = B.Cache.__new__(B.Cache)
        c._h = None
        cs.append(c)
    got = m.verify_packed(cs, [1, 2], [[3, 4], []], [5, 6], temperatures=[0.8, None], seeds=[3, None], draws_done=[7, None])
    assert [g.size for g in got] == [0, 0]
    m.decode_lookup_packed(cs, [[1, 2, 3], []], [1, 2], [3, 0], [4, 2], eos=[None, 5], max_draft=0)
    assert rec.calls == ["fl_batch_verify", "fl_batch_decode_lookup"]
