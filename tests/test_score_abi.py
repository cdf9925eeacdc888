"""The scoring entry points (fl_forward_score, fl_batch_score, fl_op_score) without a GPU: exported symbols, the fl_score layout in
ctypes and in the Rust mirror against the real header, and every argument error -- decided before the device is probed, with the
field named in fl_last_error()."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

from test_rust_shim import HEADER, layout, rust_structs

ENTRIES = ["fl_forward_score", "fl_batch_score", "fl_op_score"]
FIELDS = ["struct_size", "top_n", "targets", "target_logprob", "target_rank", "top_ids", "top_logprobs", "logits_out", "_reserved"]
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
    assert fa.abi_version() == 2 and fa.SCORE_NO_TARGET == 0xFFFFFFFF


def static_asserts(rows, size):
    lines = ['#include <stddef.h>', '#include "%s"' % HEADER,
             '_Static_assert(FL_SCORE_NO_TARGET == 0xffffffffu, "FL_SCORE_NO_TARGET");',
             '_Static_assert(sizeof(fl_score) == %d, "sizeof(fl_score)");' % size]
    for name, off, fsz in rows:
        lines.append('_Static_assert(offsetof(fl_score, %s) == %d, "fl_score.%s offset");' % (name, off, name))
        lines.append('_Static_assert(sizeof(((fl_score *)0)->%s) == %d, "fl_score.%s size");' % (name, fsz, name))
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "layout.c")
        open(c, "w").write("\n".join(lines) + "\nint main(void) { return 0; }\n")
        r = subprocess.run(["gcc", "-std=c11", "-fsyntax-only", c], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr


def test_ctypes_layout_matches_the_header(fa):
    S = fa.FlScore
    rows = [(n, getattr(S, n).offset, getattr(S, n).size) for n, _ in S._fields_]
    assert [n for n, _, _ in rows] == FIELDS
    static_asserts(rows, C.sizeof(S))


def test_rust_layout_matches_the_header():
    structs = rust_structs()
    assert "fl_score" in structs
    rows, size, _ = layout(structs["fl_score"], structs)
    assert [n for n, _, _ in rows] == FIELDS
    static_asserts(rows, size)


def sc_struct(fa, keep, top_n=2, size=None, lp=True, ids=True, lps=True, reserved=0, targets=None):
    a, r = np.zeros(4, np.float32), np.zeros(4, np.uint32)
    b, c = np.zeros((4, max(top_n, 1)), np.uint32), np.zeros((4, max(top_n, 1)), np.float32)
    tg = None if targets is None else np.asarray(targets, np.uint32)
    keep.extend([a, r, b, c, tg])
    s = fa.FlScore(C.sizeof(fa.FlScore) if size is None else size, top_n, None if tg is None else tg.ctypes.data, a.ctypes.data if lp else None,
                   r.ctypes.data, b.ctypes.data if ids else None, c.ctypes.data if lps else None, None)
    s._reserved[1] = reserved
    return s


BAD = [("struct_size", dict(size=8)), ("top_n", dict(top_n=-1)), ("top_n", dict(top_n=21)), ("target_logprob", dict(lp=False)),
       ("top_ids", dict(ids=False)), ("top_logprobs", dict(lps=False)), ("_reserved", dict(reserved=7))]


def calls(fa, st):
    """fl_forward_score and fl_batch_score with no model and no cache at all"""
    L = fa.lib()
    ids = np.zeros(4, np.uint32)
    off, pos = np.asarray([0, 4], np.uint64), np.zeros(1, np.uint64)
    yield L.fl_forward_score(None, None, ids.ctypes.data, 4, 0, st), L.fl_last_error().decode()
    yield L.fl_batch_score(None, None, 1, ids.ctypes.data, off.ctypes.data, pos.ctypes.data, st), L.fl_last_error().decode()


@pytest.mark.parametrize("field,kw", BAD)
def test_argument_errors_need_no_device(fa, field, kw):
    """With no model and no cache at all: the fl_score errors come first, and name the field."""
    keep = []
    st = sc_struct(fa, keep, **kw)
    for rc, msg in calls(fa, C.byref(st)):
        assert rc == BAD_ARGUMENT and field in msg, msg


def test_null_sc_and_good_sc_without_a_model(fa):
    keep = []
    for rc, msg in calls(fa, None):
        assert rc == BAD_ARGUMENT and "sc" in msg, msg
    for st in (sc_struct(fa, keep), sc_struct(fa, keep, top_n=0, ids=False, lps=False), sc_struct(fa, keep, targets=[1, 2, 0xFFFFFFFF, 3])):
        for rc, msg in calls(fa, C.byref(st)):                         # a well-formed fl_score: the next error is the null handle's
            assert rc == BAD_ARGUMENT and ("model" in msg or "null argument" in msg), msg


@pytest.mark.parametrize("what,T,V,targets,top_n", [("top_n", 1, 8, [0], 9), ("top_n", 1, 64, [0], 21), ("top_n", 1, 64, [0], -1),
                                                    ("targets", 2, 8, [0, 8], 2), ("T", 0, 8, [], 1), ("T", 1025, 8, [0] * 1025, 1),
                                                    ("V", 1, (1 << 24) + 1, [0], 1)])
def test_op_argument_errors_need_no_device(fa, what, T, V, targets, top_n):
    L = fa.lib()
    logits = np.zeros(max(T, 1) * min(V, 64), np.float32)               # (never read: the checks come first)
    tg = np.asarray(targets + [0], np.uint32)
    out, rk, ids, lps = np.zeros(1025, np.float32), np.zeros(1025, np.uint32), np.zeros(1025 * 20, np.uint32), np.zeros(1025 * 20, np.float32)
    rc = L.fl_op_score(logits.ctypes.data, T, V, tg.ctypes.data, top_n, out.ctypes.data, rk.ctypes.data, ids.ctypes.data, lps.ctypes.data)
    assert rc == BAD_ARGUMENT and what in L.fl_last_error().decode(), L.fl_last_error()


def test_op_missing_arrays(fa):
    L = fa.lib()
    logits, tg = np.zeros(8, np.float32), np.asarray([0xFFFFFFFF], np.uint32)      # (the sentinel is no range error)
    out, ids, lps = np.zeros(1, np.float32), np.zeros(20, np.uint32), np.zeros(20, np.float32)
    rc = L.fl_op_score(logits.ctypes.data, 1, 8, tg.ctypes.data, 2, out.ctypes.data, None, None, lps.ctypes.data)
    assert rc == BAD_ARGUMENT and "top_ids" in L.fl_last_error().decode()
    rc = L.fl_op_score(logits.ctypes.data, 1, 8, tg.ctypes.data, 0, None, None, None, None)
    assert rc == BAD_ARGUMENT and "target_logprob" in L.fl_last_error().decode()
    rc = L.fl_op_score(logits.ctypes.data, 1, 8, None, 0, out.ctypes.data, None, None, None)
    assert rc == BAD_ARGUMENT and "targets" in L.fl_last_error().decode()
