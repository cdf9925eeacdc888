"""fl_batch_prefill / fl_op_attention_packed without a GPU: the symbols are declared and exported, the ABI version did not move, the
ctypes prototypes and the Rust extern block know them, and every argument error that needs no device comes back with its code (and
a message) before the device is touched."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "fastllm_mi355x.h")
FFI = os.path.join(ROOT, "rust", "fastllm-mi355x", "src", "ffi.rs")
NEW = ("fl_batch_prefill", "fl_op_attention_packed")
BAD, NO_DEVICE, UNSUPPORTED = -8, -9, -10


@pytest.fixture(scope="module")
def L():
    import fastllm_amd
    return fastllm_amd.lib()


def test_new_symbols_are_declared_exported_and_bound(L):
    import fastllm_amd
    hdr = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    out = subprocess.check_output(["nm", "-D", "--defined-only", fastllm_amd.binding.LIB_PATH], text=True)
    exported = set(re.findall(r" T (fl_[a-z_0-9]+)", out))
    rust = open(FFI).read()
    rust = rust[rust.index('extern "C" {'):]
    for name, n_args in zip(NEW, (9, 16)):
        m = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % name, hdr, re.S)
        assert m, name + " is not declared in the header"
        assert m.group(1).count(",") + 1 == n_args, name
        assert name in exported, name
        assert len(getattr(L, name).argtypes) == n_args, name + ": ctypes prototype"
        assert re.search(r"pub fn %s\s*\(" % name, rust), name + " is not in the Rust extern block"
    assert re.search(r"#define\s+FL_ABI_VERSION\s+2\b", hdr) and L.fl_abi_version() == 2      # the change only adds entries
    assert "pub fn prefill_packed" in open(os.path.join(os.path.dirname(FFI), "safe.rs")).read()
    assert hasattr(fastllm_amd.Model, "prefill_packed") and hasattr(fastllm_amd, "op_attention_packed")


def test_batch_prefill_argument_errors_need_no_device(L):
    ids = np.array([1, 2, 3], np.uint32)
    off = np.array([0, 3], np.uint64)
    pos = np.array([0], np.uint64)
    tok = np.full(65, 7, np.uint32)
    caches = (C.c_void_p * 65)(*([0xdead0] * 65))             # never dereferenced: every call below is refused first
    fake_model = C.c_void_p(0xdead0)

    def rc(m=fake_model, c=caches, n=1, ids=ids.ctypes.data, off=off.ctypes.data, pos=pos.ctypes.data):
        return L.fl_batch_prefill(m, C.cast(c, C.c_void_p) if c is not None else None, n, ids, off, pos, None, tok.ctypes.data, None)

    for kw in (dict(m=None), dict(c=None), dict(ids=None), dict(off=None), dict(pos=None)):
        assert rc(**kw) == BAD, kw
        assert b"null" in L.fl_last_error()
    assert rc(n=0) == BAD and L.fl_last_error()
    assert b"1..64" in L.fl_last_error()
    assert rc(n=65) == BAD and b"65" in L.fl_last_error()
    assert (tok == 7).all()                                    # a refused call writes nothing


def test_op_attention_packed_argument_errors(L):
    H, Hkv, d = 6, 2, 64
    counts, past = [3, 2], [4, 0]
    q = np.zeros((5, H * d), np.uint16)
    ka = [np.zeros((2, 9, Hkv * d), np.uint16), np.zeros((2, 4, Hkv * d), np.uint16)]
    kp = (C.c_void_p * 2)(*[a.ctypes.data for a in ka])
    nullp = (C.c_void_p * 2)(ka[0].ctypes.data, None)
    out = np.full((5, H * d), 7.0, np.float32)
    i64 = lambda *x: np.array(x, np.int64)

    def rc(n=2, off=i64(0, 3, 5), past=i64(*past), rows=i64(9, 4), sa=i64(32, 64), n_layers=2, layer=1, H=H, Hkv=Hkv, d=d, window=-1, pad=0.0,
           q=q.ctypes.data, k=kp, v=kp, o=out.ctypes.data, null=()):
        a = [None if nm in null else x.ctypes.data for nm, x in (("off", off), ("past", past), ("rows", rows), ("sa", sa))]
        return L.fl_op_attention_packed(q, C.cast(k, C.c_void_p), C.cast(v, C.c_void_p), n, a[0], a[1], a[2], a[3], n_layers, layer, H, Hkv, d,
                                        window, pad, o)

    assert rc(q=None) == BAD and rc(o=None) == BAD and b"null" in L.fl_last_error()
    assert all(rc(null=(nm,)) == BAD for nm in ("off", "past", "rows", "sa"))
    assert rc(k=nullp) == BAD and rc(v=nullp) == BAD and b"sequence 1" in L.fl_last_error()
    assert rc(n=0) == BAD and rc(n_layers=0) == BAD and rc(layer=2) == BAD and rc(layer=-1) == BAD
    assert rc(off=i64(1, 3, 5)) == BAD and rc(off=i64(0, 3, 3)) == BAD                      # offsets[0] != 0; an empty sequence
    assert rc(past=i64(-1, 0)) == BAD
    # the codes fl_op_attention_batch uses
    assert rc(d=96) == UNSUPPORTED and b"head_dim" in L.fl_last_error()
    assert rc(H=7) == BAD and b"multiple of Hkv" in L.fl_last_error()
    assert rc(H=18) == UNSUPPORTED and b"at most 8" in L.fl_last_error()
    assert rc(sa=i64(32, 40)) == BAD and b"multiple of 32" in L.fl_last_error()
    assert rc(past=i64(7, 0)) == BAD and b"k_rows" in L.fl_last_error()                     # s_past + count > k_rows
    assert rc(rows=i64(9, 65)) == BAD                                                       # k_rows > seq_alloc
    assert rc(pad=float("nan")) == BAD and rc(pad=float("inf")) == BAD and b"finite" in L.fl_last_error()
    assert (out == 7.0).all()
    assert rc() in (0, NO_DEVICE)                                                           # well-formed: the device, or the loud "no device"
