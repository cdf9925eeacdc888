"""The log-prob entry points without a GPU: exported symbols, the fl_logprobs layout in ctypes and in the Rust mirror against the
real header, and every argument error -- decided before the device is probed, with the field named in fl_last_error()."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

import logprob_cases as lc
from test_rust_shim import HEADER, layout, rust_structs

ENTRIES = ["fl_forward_sample_lp", "fl_decode_sample_lp", "fl_batch_decode_each_lp", "fl_op_logprobs"]
BAD_ARGUMENT = -8


@pytest.fixture(scope="module")
def fa():
    import fastllm_amd
    return fastllm_amd


def test_symbols_are_exported(fa):
    out = subprocess.check_output(["nm", "-D", "--defined-only", fa.binding.LIB_PATH], text=True)
    for name in ENTRIES:
        assert (" T %s\\n" % name) in out.replace("\n", "\\n"), name
        assert getattr(fa.lib(), name).argtypes is not None, name
    assert fa.abi_version() == 2 and fa.LOGPROBS_MAX_TOP == 20


def static_asserts(rows, size):
    lines = ['#include <stddef.h>', '#include "%s"' % HEADER,
             '_Static_assert(FL_LOGPROBS_MAX_TOP == 20, "FL_LOGPROBS_MAX_TOP");',
             '_Static_assert(sizeof(fl_logprobs) == %d, "sizeof(fl_logprobs)");' % size]
    for name, off, fsz in rows:
        lines.append('_Static_assert(offsetof(fl_logprobs, %s) == %d, "fl_logprobs.%s offset");' % (name, off, name))
        lines.append('_Static_assert(sizeof(((fl_logprobs *)0)->%s) == %d, "fl_logprobs.%s size");' % (name, fsz, name))
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "layout.c")
        open(c, "w").write("\n".join(lines) + "\nint main(void) { return 0; }\n")
        r = subprocess.run(["gcc", "-std=c11", "-fsyntax-only", c], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr


def test_ctypes_layout_matches_the_header(fa):
    S = fa.FlLogprobs
    rows = [(n, getattr(S, n).offset, getattr(S, n).size) for n, _ in S._fields_]
    assert [n for n, _, _ in rows] == ["struct_size", "top_n", "token_logprob", "top_ids", "top_logprobs", "_reserved"]
    static_asserts(rows, C.sizeof(S))


def test_rust_layout_matches_the_header():
    structs = rust_structs()
    assert "fl_logprobs" in structs
    rows, size, _ = layout(structs["fl_logprobs"], structs)
    assert len(rows) == 6
    static_asserts(rows, size)


def lp_struct(fa, keep, top_n=2, size=None, token=True, ids=True, lps=True, reserved=0):
    a, b, c = np.zeros(4, np.float32), np.zeros((4, max(top_n, 1)), np.uint32), np.zeros((4, max(top_n, 1)), np.float32)
    keep.extend([a, b, c])
    s = fa.FlLogprobs(C.sizeof(fa.FlLogprobs) if size is None else size, top_n, a.ctypes.data if token else None, b.ctypes.data if ids else None,
                      c.ctypes.data if lps else None)
    s._reserved[1] = reserved
    return s


BAD = [("struct_size", dict(size=8)), ("top_n", dict(top_n=-1)), ("top_n", dict(top_n=21)), ("token_logprob", dict(token=False)),
       ("top_ids", dict(ids=False)), ("top_logprobs", dict(lps=False)), ("_reserved", dict(reserved=7))]


@pytest.mark.parametrize("field,kw", BAD)
def test_argument_errors_need_no_device(fa, field, kw):
    """With no model and no cache at all: the fl_logprobs errors come first, and name the field."""
    L, keep = fa.lib(), []
    st = lp_struct(fa, keep, **kw)
    tok, n = C.c_uint32(0), C.c_size_t(0)
    ids = np.zeros(4, np.uint32)
    rc = L.fl_forward_sample_lp(None, None, ids.ctypes.data, 4, 0, None, C.byref(tok), C.byref(st))
    assert rc == BAD_ARGUMENT and field in L.fl_last_error().decode(), L.fl_last_error()
    rc = L.fl_decode_sample_lp(None, None, 1, 0, 4, -1, None, ids.ctypes.data, C.byref(n), C.byref(st))
    assert rc == BAD_ARGUMENT and field in L.fl_last_error().decode(), L.fl_last_error()


def test_null_lp_and_good_lp_without_a_model(fa):
    L, keep = fa.lib(), []
    tok, n = C.c_uint32(0), C.c_size_t(0)
    ids = np.zeros(4, np.uint32)
    assert L.fl_forward_sample_lp(None, None, ids.ctypes.data, 4, 0, None, C.byref(tok), None) == BAD_ARGUMENT and "lp" in L.fl_last_error().decode()
    assert L.fl_decode_sample_lp(None, None, 1, 0, 4, -1, None, ids.ctypes.data, C.byref(n), None) == BAD_ARGUMENT and "lp" in L.fl_last_error().decode()
    assert L.fl_batch_decode_each_lp(None, ids.ctypes.data, None, 4, None, None, ids.ctypes.data, None, None) == BAD_ARGUMENT and "lp" in L.fl_last_error().decode()
    st = lp_struct(fa, keep)                                            # a well-formed fl_logprobs: the next error is the null model's
    assert L.fl_forward_sample_lp(None, None, ids.ctypes.data, 4, 0, None, C.byref(tok), C.byref(st)) == BAD_ARGUMENT
    assert L.fl_batch_decode_each_lp(None, ids.ctypes.data, None, 4, None, None, ids.ctypes.data, None, C.byref(st)) == BAD_ARGUMENT
    st0 = lp_struct(fa, keep, top_n=0, ids=False, lps=False)            # top_n == 0 needs no top arrays
    rc = L.fl_forward_sample_lp(None, None, ids.ctypes.data, 4, 0, None, C.byref(tok), C.byref(st0))
    assert rc == BAD_ARGUMENT and "model" in L.fl_last_error().decode()


@pytest.mark.parametrize("what,T,V,chosen,top_n", [("top_n", 1, 8, [0], 9), ("top_n", 1, 64, [0], 21), ("top_n", 1, 64, [0], -1), ("chosen", 2, 8, [0, 8], 2),
                                                   ("T", 0, 8, [], 1), ("T", 65, 8, [0] * 65, 1), ("V", 1, (1 << 24) + 1, [0], 1)])
def test_op_argument_errors_need_no_device(fa, what, T, V, chosen, top_n):
    L = fa.lib()
    logits = np.zeros(max(T, 1) * min(V, 64), np.float32)               # (never read: the checks come first)
    ch = np.asarray(chosen + [0], np.uint32)
    out, ids, lps = np.zeros(65, np.float32), np.zeros(65 * 20, np.uint32), np.zeros(65 * 20, np.float32)
    rc = L.fl_op_logprobs(logits.ctypes.data, T, V, ch.ctypes.data, top_n, out.ctypes.data, ids.ctypes.data, lps.ctypes.data)
    assert rc == BAD_ARGUMENT and what in L.fl_last_error().decode(), L.fl_last_error()
    rc = L.fl_op_logprobs(logits.ctypes.data, 1, 8, ch.ctypes.data, 2, out.ctypes.data, None, lps.ctypes.data)
    assert rc == BAD_ARGUMENT and "top_ids" in L.fl_last_error().decode()


def test_tolerance_holds_for_a_float32_restatement():
    """The bound the GPU tests use is derived, not measured: a numpy float32 restatement of the prescribed arithmetic (fp32
    subtraction, fp32 exp, fp64 sum, fp32 log and subtraction) stays within it on every row of the kernel test."""
    for name, (a, _) in lc.rows().items():
        for t in range(a.shape[0]):
            lp, _ = lc.ref_logprobs(a[t])
            got, bound = lc.f32_restatement(a[t]), lc.tol(a[t], lp)
            fin = np.isfinite(lp)
            assert np.array_equal(got[~fin], lp[~fin]), name
            assert (np.abs(got[fin] - lp[fin]) <= bound[fin]).all(), (name, t)
