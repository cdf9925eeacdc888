"""Decoder-model embeddings without a GPU: fl_embed has the header's layout, the new entry points are exported and declared, the ABI
version is still 2, and every argument error that needs neither a model nor a device comes back as FL_ERR_BAD_ARGUMENT naming the
field -- before the handles are looked at (they are NULL here: no model can exist without a GPU) and before the device is probed."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "fastllm_mi355x.h")
NEW = ("fl_batch_embed", "fl_op_pool_rows", "fl_op_pool_rows_time", "fl_op_attention_packed_ex")


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
    assert re.search(r"#define\s+FL_ABI_VERSION\s+2\b", hdr) and L.fl_abi_version() == 2     # the change only adds entries


def test_fl_embed_layout_and_enums_match_the_header():
    import fastllm_amd.binding as B
    fields = ["struct_size", "pooling", "mask", "normalize", "dimensions", "_reserved"]
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "s.c"), os.path.join(d, "s")
        body = 'printf("%zu", sizeof(fl_embed));' +"".join(' printf(" %%zu", offsetof(fl_embed, %s));' % f for f in fields)
        body += ' printf(" %d %d %d %d %d %d", FL_POOL_LAST, FL_POOL_MEAN, FL_POOL_FIRST, FL_POOL_NONE, FL_MASK_CAUSAL, FL_MASK_FULL);'
        open(src, "w").write('#include <stdio.h>\n#include <stddef.h>\n#include "%s"\nint main(void) { %s return 0; }\n' % (HEADER, body))
        subprocess.run(["gcc", "-std=c11", src, "-o", exe], check=True)
        vals = [int(x) for x in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert vals[0] == C.sizeof(B.FlEmbed) == 40
    assert vals[1:7] == [getattr(B.FlEmbed, f).offset for f in fields] == [0, 4, 8, 12, 16, 24]
    assert vals[7:] == [B.POOLING["last"], B.POOLING["mean"], B.POOLING["first"], B.POOLING["none"], B.ATTN_MASK["causal"], B.ATTN_MASK["full"]]
    assert vals[7:] == [0, 1, 2, 3, 0, 1]


def bad_structs(B):
    """(fl_embed with one fault, the word its message must hold)"""
    def make(**kw):
        e = B.make_embed()
        for k, v in kw.items():
            setattr(e, k, v)
        return e
    r0, r1 = B.make_embed(), B.make_embed()
    r0._reserved[0], r1._reserved[1] = 1, -1
    return [(make(struct_size=32), b"struct_size"), (make(struct_size=48), b"struct_size"), (make(pooling=4), b"pooling"),
            (make(pooling=-1), b"pooling"), (make(mask=2), b"mask"), (make(mask=-1), b"mask"), (make(normalize=2), b"normalize"),
            (make(normalize=-1), b"normalize"), (make(dimensions=-1), b"dimensions"), (r0, b"_reserved"), (r1, b"_reserved")]


def test_fl_batch_embed_argument_errors_come_before_the_handles(L):
    import fastllm_amd.binding as B
    ids = np.array([1, 2, 3], np.uint32)
    off = np.array([0, 3], np.uint64)
    pos = np.zeros(1, np.uint64)
    out = np.full(8, 7.0, np.float32)

    def rc(e, outp=out.ctypes.data):
        return L.fl_batch_embed(None, None, 1, ids.ctypes.data, off.ctypes.data, pos.ctypes.data, C.byref(e) if e is not None else None, outp)

    for e, word in bad_structs(B):
        assert rc(e) == -8 and word in L.fl_last_error(), (word, L.fl_last_error())
    assert rc(None) == -8 and b"null fl_embed" in L.fl_last_error()
    assert rc(B.make_embed(), outp=None) == -8 and b"null out" in L.fl_last_error()
    # a well-formed struct: the only fault left is the missing model
    assert rc(B.make_embed("mean", "full", False, 40)) == -8 and b"null argument" in L.fl_last_error()
    assert (out == 7.0).all()                                # nothing was written


def test_fl_op_pool_rows_argument_errors_come_before_the_device(L):
    import fastllm_amd.binding as B
    x = np.zeros((3, 8), np.float32)
    inv = np.ones(3, np.float32)
    w = np.ones(8, np.float32)
    off = np.array([0, 1, 3], np.uint64)
    out = np.zeros((3, 8), np.float32)

    def rc(e, xp=x.ctypes.data, offs=off, h=8, n=2, outp=out.ctypes.data):
        return L.fl_op_pool_rows(xp, inv.ctypes.data, w.ctypes.data, offs.ctypes.data, n, h, C.byref(e) if e is not None else None, outp)

    for e, word in bad_structs(B):
        assert rc(e) == -8 and word in L.fl_last_error(), (word, L.fl_last_error())
    assert rc(None) == -8
    assert rc(B.make_embed(), xp=None) == -8 and rc(B.make_embed(), outp=None) == -8
    assert rc(B.make_embed(dimensions=9)) == -8 and b"dimensions" in L.fl_last_error()      # beyond h
    assert rc(B.make_embed(), h=0) == -8 and rc(B.make_embed(), n=0) == -8
    assert rc(B.make_embed(), offs=np.array([0, 2, 2], np.uint64)) == -8 and b"offsets" in L.fl_last_error()   # an empty member
    assert rc(B.make_embed(), offs=np.array([1, 2, 3], np.uint64)) == -8
    ms = C.c_double(0)
    assert L.fl_op_pool_rows_time(x.ctypes.data, inv.ctypes.data, w.ctypes.data, off.ctypes.data, 2, 8, C.byref(B.make_embed()), 0, C.byref(ms)) == -8
    assert rc(B.make_embed("mean", 0, True, 5)) in (0, -9)   # a well-formed call reaches the device, or the loud "no device"


def test_fl_op_attention_packed_ex_refuses_an_unknown_mask(L):
    q = np.zeros((1, 128), np.uint16)
    one = np.zeros(1, np.int64)
    assert L.fl_op_attention_packed_ex(q.ctypes.data, None, None, 1, one.ctypes.data, one.ctypes.data, one.ctypes.data, one.ctypes.data, 1, 0, 2, 2, 64, -1,
                                       0.0, 2, q.ctypes.data) == -8
    assert b"mask" in L.fl_last_error()
