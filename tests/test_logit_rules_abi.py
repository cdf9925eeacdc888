"""The logit-rules entry points without a GPU: exported symbols, the fl_logit_rules layout in ctypes and in the Rust mirror against
the real header, every argument error of fl_cache_set_logit_rules that can be decided without a model -- all of them before the
device is probed, with the field named in fl_last_error() -- and the numpy restatement the GPU tests compare against, checked on
hand-worked rows.  (An id >= V needs a model to know V: tests/test_gpu_logit_rules.py has that refusal.)"""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

import logit_rules_ref as lr
from test_rust_shim import HEADER, layout, rust_structs

ENTRIES = ["fl_cache_set_logit_rules", "fl_cache_logit_counts", "fl_op_logit_rules"]
BAD_ARGUMENT = -8
FIELDS = ["struct_size", "n_bias", "bias_ids", "bias_values", "repetition_penalty", "frequency_penalty", "presence_penalty", "_reserved"]


@pytest.fixture(scope="module")
def fa():
    import fastllm_amd
    return fastllm_amd


def test_symbols_are_exported(fa):
    out = subprocess.check_output(["nm", "-D", "--defined-only", fa.binding.LIB_PATH], text=True)
    for name in ENTRIES:
        assert (" T %s\n" % name) in out, name
        assert getattr(fa.lib(), name).argtypes is not None, name
    assert fa.abi_version() == 2


def static_asserts(rows, size):
    lines = ['#include <stddef.h>', '#include "%s"' % HEADER, '_Static_assert(sizeof(fl_logit_rules) == %d, "sizeof(fl_logit_rules)");' % size]
    for name, off, fsz in rows:
        lines.append('_Static_assert(offsetof(fl_logit_rules, %s) == %d, "fl_logit_rules.%s offset");' % (name, off, name))
        lines.append('_Static_assert(sizeof(((fl_logit_rules *)0)->%s) == %d, "fl_logit_rules.%s size");' % (name, fsz, name))
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "layout.c")
        open(c, "w").write("\n".join(lines) + "\nint main(void) { return 0; }\n")
        r = subprocess.run(["gcc", "-std=c11", "-fsyntax-only", c], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr


def test_ctypes_layout_matches_the_header(fa):
    S = fa.FlLogitRules
    rows = [(n, getattr(S, n).offset, getattr(S, n).size) for n, _ in S._fields_]
    assert [n for n, _, _ in rows] == FIELDS
    static_asserts(rows, C.sizeof(S))


def test_rust_layout_matches_the_header():
    structs = rust_structs()
    assert "fl_logit_rules" in structs
    rows, size, _ = layout(structs["fl_logit_rules"], structs)
    assert [n for n, _, _ in rows] == FIELDS
    static_asserts(rows, size)


def rules(fa, keep, ids=(1, 2), vals=(0.5, -1.0), rp=1.0, fp=0.0, pp=0.0, size=None, reserved=0, null_ids=False, null_vals=False):
    i, v = np.asarray(ids, np.uint32), np.asarray(vals, np.float32)
    keep.extend([i, v])
    st = fa.FlLogitRules(C.sizeof(fa.FlLogitRules) if size is None else size, len(ids), None if null_ids else i.ctypes.data,
                         None if null_vals else v.ctypes.data, rp, fp, pp)
    st._reserved[1] = reserved
    return st


BAD = [("struct_size", dict(size=16)), ("_reserved", dict(reserved=3)),
       ("repetition_penalty", dict(rp=float("nan"))), ("repetition_penalty", dict(rp=0.0)), ("repetition_penalty", dict(rp=-1.5)),
       ("repetition_penalty", dict(rp=float("inf"))), ("frequency_penalty", dict(fp=float("nan"))), ("frequency_penalty", dict(fp=float("inf"))),
       ("presence_penalty", dict(pp=float("nan"))), ("presence_penalty", dict(pp=float("-inf"))),
       ("bias_values", dict(vals=(0.5, float("nan")))), ("bias_values", dict(vals=(float("inf"), 0.0))),
       ("duplicate", dict(ids=(7, 3, 7), vals=(0.0, 0.0, 0.0))), ("bias_ids", dict(null_ids=True)), ("bias_values", dict(null_vals=True))]


@pytest.mark.parametrize("field,kw", BAD)
def test_argument_errors_need_no_device(fa, field, kw):
    """With no model and no cache at all: the fl_logit_rules errors come first, and name the field."""
    L, keep = fa.lib(), []
    st = rules(fa, keep, **kw)
    ids = np.zeros(4, np.uint32)
    rc = L.fl_cache_set_logit_rules(None, None, C.byref(st), ids.ctypes.data, 4, ids.ctypes.data, 4)
    assert rc == BAD_ARGUMENT and field in L.fl_last_error().decode(), L.fl_last_error()


def test_null_lists_and_good_rules_without_a_model(fa):
    L, keep = fa.lib(), []
    ids = np.zeros(4, np.uint32)
    st = rules(fa, keep)
    assert L.fl_cache_set_logit_rules(None, None, C.byref(st), None, 4, ids.ctypes.data, 4) == BAD_ARGUMENT and "prompt_ids" in L.fl_last_error().decode()
    assert L.fl_cache_set_logit_rules(None, None, C.byref(st), ids.ctypes.data, 4, None, 2) == BAD_ARGUMENT and "output_ids" in L.fl_last_error().decode()
    # -inf is a legal bias, and empty lists may be null: the next error is the null model's
    ok = rules(fa, keep, vals=(float("-inf"), 2.0), rp=1.3, fp=-0.5, pp=0.25)
    assert L.fl_cache_set_logit_rules(None, None, C.byref(ok), None, 0, None, 0) == BAD_ARGUMENT and "model" in L.fl_last_error().decode()
    empty = rules(fa, keep, ids=(), vals=(), null_ids=True, null_vals=True)
    assert L.fl_cache_set_logit_rules(None, None, C.byref(empty), None, 0, None, 0) == BAD_ARGUMENT and "model" in L.fl_last_error().decode()
    assert L.fl_cache_set_logit_rules(None, None, None, None, 0, None, 0) == BAD_ARGUMENT and "model" in L.fl_last_error().decode()   # a removal
    assert L.fl_cache_logit_counts(None, None, ids.ctypes.data) == BAD_ARGUMENT


@pytest.mark.parametrize("what,B,V", [("B", 0, 8), ("B", 65, 8), ("V", 1, 0), ("V", 1, (1 << 24) + 1)])
def test_op_argument_errors_need_no_device(fa, what, B, V):
    L = fa.lib()
    a = np.zeros(64 * 8, np.float32)                                    # (never read: the checks come first)
    w = np.zeros(64 * 8, np.uint32)
    rc = L.fl_op_logit_rules(a.ctypes.data, B, V, w.ctypes.data, a.ctypes.data, a.ctypes.data, w.ctypes.data, 1, None, a.ctypes.data)
    assert rc == BAD_ARGUMENT and what in L.fl_last_error().decode(), L.fl_last_error()
    assert L.fl_op_logit_rules(a.ctypes.data, 1, 8, None, a.ctypes.data, a.ctypes.data, w.ctypes.data, 1, None, a.ctypes.data) == BAD_ARGUMENT


def test_reference_helper_on_hand_worked_rows():
    P = int(lr.PROMPT_BIT)
    inf = float("inf")
    f13 = 1.2999999523162842                                            # float32(1.3)
    #        x      word    bias   want (rp = 1.3, fp = 0.5, pp = 0.25)
    rows = [(0.0,   P,      0.0,   0.0),                                # x = 0 stays 0 under the repetition penalty
            (-2.0,  P,      0.0,   -2.0 * f13),                         # a negative logit is MULTIPLIED: -2 * float32(1.3), exact
            (2.0,   0,      0.0,   2.0),                                # an id never seen: untouched
            (2.0,   0,      -inf,  -inf),                               # a banned id
            (-inf,  P | 2,  1.0,   -inf),                               # a -inf logit stays -inf through every rule
            (4.0,   0,      0.5,   4.5)]                                # bias alone
    x, words, bias, want = (np.asarray(c) for c in zip(*rows))
    got = lr.apply(x.astype(np.float32), words.astype(np.uint32), bias.astype(np.float32), 1.3, 0.5, 0.25)
    assert got.dtype == np.float32 and np.array_equal(lr.bits(got), lr.bits(want.astype(np.float32))), got
    # counts: 3 / 1.5 = 2, - 1 * 0.5 = 1.5, - 0.25 = 1.25, + 0.5 = 1.75 (every step exact in float32)
    assert lr.apply([3.0], [1], [0.5], 1.5, 0.5, 0.25)[0] == np.float32(1.75)
    # c = 3 with a NEGATIVE frequency penalty rewards repetition: 1 - 3 * (-0.5) = 2.5, - 0.25 = 2.25; rp = 1 leaves the prompt bit without effect
    assert lr.apply([1.0, 1.0], [3, P], [0.0, 0.0], 1.0, -0.5, 0.25).tolist() == [2.25, 1.0]
    # each operation is rounded on its own: 0.1 / 1.3 in float32, then the float32 product 7 * 0.3 subtracted
    one = lr.apply([0.1], [7], [0.0], 1.3, 0.3, 0.0)[0]
    assert one == np.float32(np.float32(np.float32(0.1) / np.float32(1.3)) - np.float32(np.float32(7) * np.float32(0.3)))
    # the table and the counting
    w, b = lr.table(8, prompt_ids=[1, 1, 5], output_ids=[5, 5, 2], logit_bias={3: -inf, 0: 1.5})
    assert w.tolist() == [0, P, 1, 0, 0, P | 2, 0, 0] and b.tolist() == [1.5, 0, 0, -inf, 0, 0, 0, 0]
    assert lr.count(w, 1)[1] == P | 1 and lr.count(w, 99).tolist() == w.tolist()
    assert lr.argmax_last(np.asarray([1.0, 3.0, 3.0, -inf], np.float32)) == 2
