"""The guided-decoding entry points without a GPU: exported symbols, the fl_guide_desc layout in ctypes and in the Rust mirror against
the real header, and every argument error of fl_guide_create that can be decided without a model -- all of them before the device is
probed (this test runs where there is none), with the reason in fl_last_error().  (An id >= V needs a model to know V:
fl_op_guide_mask, which takes V, shows that refusal here; tests/test_gpu_guide.py has the model's.)"""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

from test_rust_shim import HEADER, layout, rust_structs

ENTRIES = ["fl_guide_create", "fl_guide_destroy", "fl_cache_set_guide", "fl_cache_guide_state", "fl_op_guide_mask"]
BAD_ARGUMENT = -8
FIELDS = ["struct_size", "n_states", "row_ptr", "tokens", "next", "_reserved"]


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
    lines = ['#include <stddef.h>', '#include "%s"' % HEADER, '_Static_assert(sizeof(fl_guide_desc) == %d, "sizeof(fl_guide_desc)");' % size]
    for name, off, fsz in rows:
        lines.append('_Static_assert(offsetof(fl_guide_desc, %s) == %d, "fl_guide_desc.%s offset");' % (name, off, name))
        lines.append('_Static_assert(sizeof(((fl_guide_desc *)0)->%s) == %d, "fl_guide_desc.%s size");' % (name, fsz, name))
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "layout.c")
        open(c, "w").write("\n".join(lines) + "\nint main(void) { return 0; }\n")
        r = subprocess.run(["gcc", "-std=c11", "-fsyntax-only", c], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr


def test_ctypes_layout_matches_the_header(fa):
    S = fa.FlGuideDesc
    rows = [(n, getattr(S, n).offset, getattr(S, n).size) for n, _ in S._fields_]
    assert [n for n, _, _ in rows] == FIELDS
    static_asserts(rows, C.sizeof(S))


def test_rust_layout_matches_the_header():
    structs = rust_structs()
    assert "fl_guide_desc" in structs
    rows, size, _ = layout(structs["fl_guide_desc"], structs)
    assert [n for n, _, _ in rows] == FIELDS
    static_asserts(rows, size)


# two states over ids 0..9: state 0 allows {1, 4, 7} -> 1, state 1 allows {0, 9} -> 0
GOOD = dict(row_ptr=[0, 3, 5], tokens=[1, 4, 7, 0, 9], next=[1, 1, 1, 0, 0])


def desc(fa, keep, size=None, reserved=0, n_states=None, null=None, **kw):
    d = dict(GOOD, **kw)
    st, arrays = fa.make_guide_desc(d["row_ptr"], d["tokens"], d["next"])
    keep.append(arrays)
    if size is not None:
        st.struct_size = size
    if n_states is not None:
        st.n_states = n_states
    if null:
        setattr(st, null, None)
    st._reserved[1] = reserved
    return st


BAD = [("no edge", dict(row_ptr=[0, 3, 3, 5], next=[1, 1, 1, 0, 0])),              # state 1 is empty
       ("ascending", dict(tokens=[4, 1, 7, 0, 9])),                               # unsorted within a state
       ("ascending", dict(tokens=[1, 4, 4, 0, 9])),                               # a duplicate within a state
       ("next", dict(next=[1, 1, 2, 0, 0])),                                      # next >= n_states
       ("row_ptr", dict(row_ptr=[1, 3, 5])),                                      # does not start at 0
       ("row_ptr", dict(row_ptr=[0, 4, 3, 5], next=[1, 1, 1, 0, 0])),             # decreases
       ("struct_size", dict(size=16)), ("_reserved", dict(reserved=3)), ("n_states", dict(n_states=0)),
       ("null", dict(null="row_ptr")), ("null", dict(null="tokens")), ("null", dict(null="next"))]


@pytest.mark.parametrize("reason,kw", BAD)
def test_argument_errors_need_no_device(fa, reason, kw):
    """With no model at all: the fl_guide_desc errors come first, and say what is wrong."""
    L, keep = fa.lib(), []
    st = desc(fa, keep, **kw)
    out = C.c_void_p(0x1234)
    rc = L.fl_guide_create(None, C.byref(st), C.byref(out))
    assert rc == BAD_ARGUMENT and reason in L.fl_last_error().decode(), L.fl_last_error()
    assert out.value is None                                            # no guide came of it


def test_good_desc_and_null_handles_without_a_model(fa):
    L, keep = fa.lib(), []
    out = C.c_void_p()
    ok = desc(fa, keep)
    assert L.fl_guide_create(None, C.byref(ok), C.byref(out)) == BAD_ARGUMENT and "model" in L.fl_last_error().decode()
    assert L.fl_guide_create(None, None, C.byref(out)) == BAD_ARGUMENT and "desc" in L.fl_last_error().decode()
    assert L.fl_guide_create(None, C.byref(ok), None) == BAD_ARGUMENT
    assert L.fl_cache_set_guide(None, None, None, 0) == BAD_ARGUMENT and "model" in L.fl_last_error().decode()
    state = C.c_uint32(0)
    assert L.fl_cache_guide_state(None, C.byref(state)) == BAD_ARGUMENT
    L.fl_guide_destroy(None)                                            # a null handle is ignored


def test_op_argument_errors_need_no_device(fa):
    L, keep = fa.lib(), []
    a = np.zeros(64 * 10, np.float32)                                   # (never read: the checks come first)
    s = np.zeros(64, np.uint32)
    ok = desc(fa, keep)

    def op(B, V, st, states=s):
        return L.fl_op_guide_mask(a.ctypes.data, B, V, C.byref(st), states.ctypes.data, s.ctypes.data, None, a.ctypes.data, s.ctypes.data)
    for what, B, V in [("B", 0, 10), ("B", 65, 10), ("V", 1, 0), ("V", 1, (1 << 24) + 1)]:
        assert op(B, V, ok) == BAD_ARGUMENT and what in L.fl_last_error().decode(), L.fl_last_error()
    assert op(1, 9, ok) == BAD_ARGUMENT and "out of range" in L.fl_last_error().decode()        # id 9 with V = 9
    assert op(1, 10, desc(fa, keep, tokens=[4, 1, 7, 0, 9])) == BAD_ARGUMENT and "ascending" in L.fl_last_error().decode()
    assert op(2, 10, ok, np.asarray([1, 2], np.uint32)) == BAD_ARGUMENT and "states" in L.fl_last_error().decode()
    assert L.fl_op_guide_mask(None, 1, 10, C.byref(ok), s.ctypes.data, s.ctypes.data, None, a.ctypes.data, s.ctypes.data) == BAD_ARGUMENT
