"""fl_op_attention_plain / fl_op_attention_batch without a GPU: the symbols are exported and declared, every documented argument
error comes back with its code before the device is touched, and a well-formed call on a machine without a device is the loud
FL_ERR_NO_DEVICE."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "fastllm_mi355x.h")
NEW = ("fl_op_attention_plain", "fl_op_attention_batch")
BAD, NO_DEVICE, UNSUPPORTED = -8, -9, -10
F32, BF16 = 0, 1


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
    assert re.search(r"#define\s+FL_ABI_VERSION\s+2\b", hdr) and L.fl_abi_version() == 2      # the change only adds entries
    # fl_op_attention keeps its twelve parameters
    assert re.search(r"\bfl_op_attention\s*\(([^;]*?)\)\s*;", hdr, re.S).group(1).count(",") == 11


def test_plain_argument_errors(L):
    T, s_past, H, Hkv, d = 2, 3, 6, 2, 64
    q = np.zeros((T, H * d), np.float32)
    k = np.zeros((s_past + T + 1, Hkv * d), np.float32)
    out = np.full((2, T, H * d), 7.0, np.float32)

    def rc(dtype=F32, layout=0, kernel=0, T=T, s_past=s_past, call0=1, rows=s_past + T + 1, cap=40, H=H, Hkv=Hkv, d=d, window=-1, nsplit=1,
           pad=0.0, repeat=2, q=q.ctypes.data, k=k.ctypes.data, v=k.ctypes.data, o=out.ctypes.data):
        return L.fl_op_attention_plain(q, k, v, dtype, layout, kernel, T, s_past, call0, rows, cap, H, Hkv, d, window, nsplit, pad, repeat, o)

    assert rc(q=None) == BAD and rc(k=None) == BAD and rc(v=None) == BAD and rc(o=None) == BAD and b"null" in L.fl_last_error()
    assert rc(T=0) == BAD and rc(s_past=-1) == BAD and rc(call0=-1) == BAD
    assert rc(call0=s_past + 1) == BAD and b"call0 <= s_past" in L.fl_last_error()
    assert rc(kernel=-1) == BAD and rc(kernel=4) == BAD and rc(kernel=3) == BAD              # the plain layout has one prefill kernel
    assert rc(kernel=1) == BAD and b"one query token" in L.fl_last_error()                   # decode with T = 2
    assert rc(nsplit=-1) == BAD and rc(nsplit=65) == BAD and rc(repeat=0) == BAD and rc(repeat=17) == BAD
    assert rc(rows=s_past + T - 1) == BAD and rc(cap=s_past + T) == BAD and b"k_rows <= capacity" in L.fl_last_error()
    assert rc(pad=float("nan")) == BAD and rc(pad=float("inf")) == BAD and b"finite" in L.fl_last_error()
    assert rc(dtype=2) == BAD and rc(layout=2) == BAD and rc(layout=-1) == BAD
    assert rc(H=0) == BAD and rc(Hkv=0) == BAD and rc(H=7) == BAD and b"multiple of Hkv" in L.fl_last_error()
    assert rc(d=96) == UNSUPPORTED and b"head_dim" in L.fl_last_error()
    assert rc(layout=1) == UNSUPPORTED                                                       # the MFMA kernels are bf16
    assert rc(layout=1, dtype=BF16, H=18) == UNSUPPORTED and b"at most 8" in L.fl_last_error()
    assert (out == 7.0).all()                                                                # a refused call writes nothing
    assert rc() in (0, NO_DEVICE) and rc(layout=1, dtype=BF16, kernel=3) in (0, NO_DEVICE)   # well-formed: the device, or the loud "no device"


def test_batch_argument_errors(L):
    B, H, Hkv, d = 2, 6, 2, 64
    q = np.zeros((B, H * d), np.float32)
    ka = [np.zeros((2, 5, Hkv * d), np.float32), np.zeros((2, 9, Hkv * d), np.float32)]
    kp = (C.c_void_p * B)(*[a.ctypes.data for a in ka])
    nullp = (C.c_void_p * B)(ka[0].ctypes.data, None)
    out = np.full((B, H * d), 7.0, np.float32)
    i64 = lambda *x: np.array(x, np.int64)

    def rc(dtype=F32, layout=0, B=B, lens=i64(4, 9), rows=i64(5, 9), sa=i64(32, 64), ns=np.array([0, 3], np.int32), n_layers=2, layer=1, H=H,
           Hkv=Hkv, d=d, pad=0.0, repeat=1, q=q.ctypes.data, k=kp, v=kp, o=out.ctypes.data, null=()):
        a = [None if n in null else x.ctypes.data for n, x in (("lens", lens), ("rows", rows), ("sa", sa), ("ns", ns))]
        return L.fl_op_attention_batch(q, C.cast(k, C.c_void_p), C.cast(v, C.c_void_p), dtype, layout, B, a[0], a[1], a[2], a[3], n_layers, layer,
                                       H, Hkv, d, pad, repeat, o)

    assert rc(q=None) == BAD and rc(o=None) == BAD and b"null" in L.fl_last_error()
    assert all(rc(null=(n,)) == BAD for n in ("lens", "rows", "sa", "ns"))
    assert rc(k=nullp) == BAD and rc(v=nullp) == BAD and b"sequence 1" in L.fl_last_error()
    assert rc(B=0) == BAD and rc(n_layers=0) == BAD and rc(layer=2) == BAD and rc(layer=-1) == BAD and rc(repeat=0) == BAD and rc(repeat=17) == BAD
    assert rc(lens=i64(0, 9)) == BAD and rc(lens=i64(6, 9)) == BAD                           # an empty sequence; len > k_rows
    assert rc(sa=i64(32, 40)) == BAD and b"multiple of 32" in L.fl_last_error()
    assert rc(rows=i64(5, 65)) == BAD                                                        # k_rows > seq_alloc
    assert rc(ns=np.array([0, 65], np.int32)) == BAD and rc(ns=np.array([-1, 3], np.int32)) == BAD
    assert rc(pad=float("nan")) == BAD and rc(dtype=2) == BAD and rc(layout=2) == BAD and rc(H=7) == BAD
    assert rc(d=96) == UNSUPPORTED and rc(layout=1) == UNSUPPORTED and rc(layout=1, dtype=BF16, H=18) == UNSUPPORTED
    assert (out == 7.0).all()
    assert rc() in (0, NO_DEVICE)


def test_a_valid_call_without_a_device_is_no_device(L):
    n = C.c_int(-1)
    assert L.fl_device_count(C.byref(n)) == 0
    want = 0 if n.value > 0 else NO_DEVICE                      # (with a GPU present the same calls run on it)
    q = np.zeros((1, 64), np.float32)
    k = np.zeros((1, 1, 64), np.float32)
    out = np.zeros((1, 64), np.float32)
    assert L.fl_op_attention_plain(q.ctypes.data, k.ctypes.data, k.ctypes.data, F32, 0, 0, 1, 0, 0, 1, 1, 1, 1, 64, -1, 1, 0.0, 1,
                                   out.ctypes.data) == want
    assert want == 0 or b"no HIP device" in L.fl_last_error()
    kp = (C.c_void_p * 1)(k.ctypes.data)
    one, sa, ns = np.array([1], np.int64), np.array([32], np.int64), np.array([0], np.int32)
    assert L.fl_op_attention_batch(q.ctypes.data, C.cast(kp, C.c_void_p), C.cast(kp, C.c_void_p), F32, 0, 1, one.ctypes.data, one.ctypes.data,
                                   sa.ctypes.data, ns.ctypes.data, 1, 0, 1, 1, 64, 0.0, 1, out.ctypes.data) == want
