"""The norm op entry points without a GPU: fl_op_rmsnorm_add / fl_op_norm_linear / fl_op_linear_resid are exported and declared, their
argument structs have the header's layout, and their argument errors come back before the device is touched."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "fastllm_mi355x.h")
NEW = ("fl_op_rmsnorm_add", "fl_op_norm_linear", "fl_op_linear_resid")
BAD, NO_DEVICE, UNSUPPORTED = -8, -9, -10


@pytest.fixture(scope="module")
def fa():
    import fastllm_amd
    return fastllm_amd


@pytest.fixture(scope="module")
def L(fa):
    return fa.lib()


def test_new_symbols_are_exported_and_declared(fa, L):
    hdr = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name in NEW:
        assert hasattr(L, name), name
        assert re.search(r"\b%s\s*\(" % name, hdr), name
    out = subprocess.check_output(["nm", "-D", "--defined-only", fa.binding.LIB_PATH], text=True)
    assert set(NEW) <= set(re.findall(r" T (fl_[a-z_0-9]+)", out))
    assert re.search(r"#define\s+FL_ABI_VERSION\s+2\b", hdr) and L.fl_abi_version() == 2      # the change only adds entries


def test_argument_structs_have_the_header_layout(fa):
    """every field of the two ctypes mirrors at the header's offset, and the kernel codes in the header's order"""
    b = fa.binding
    lines = ['#include <stddef.h>', '#include "%s"' % HEADER]
    for cname, st in (("fl_norm_linear_args", b.FlNormLinearArgs), ("fl_linear_resid_args", b.FlLinearResidArgs)):
        lines.append('_Static_assert(sizeof(%s) == %d, "sizeof(%s)");' % (cname, C.sizeof(st), cname))
        for name, _ in st._fields_:
            lines.append('_Static_assert(offsetof(%s, %s) == %d, "%s.%s");' % (cname, name, getattr(st, name).offset, cname, name))
    for code, name in enumerate(b.LK_NAMES):
        lines.append('_Static_assert(FL_LK_%s == %d, "FL_LK_%s");' % (name.upper(), code, name.upper()))
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "layout.c")
        open(c, "w").write("\n".join(lines) + "\nint main(void) { return 0; }\n")
        r = subprocess.run(["gcc", "-std=c11", "-fsyntax-only", c], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr


def test_rmsnorm_add_argument_errors(L):
    x, w = np.ones((2, 16), np.float32), np.ones(16, np.float32)
    d = np.ones((3, 2, 16), np.float32)
    xs, inv = np.zeros((2, 16), np.float32), np.zeros(2, np.float32)

    def rc(xp=x.ctypes.data, dp=None, n_slab=0, wp=w.ctypes.data, T=2, h=16, dtype=1, xsp=xs.ctypes.data, ip=inv.ctypes.data):
        return L.fl_op_rmsnorm_add(xp, dp, n_slab, wp, 1e-5, T, h, dtype, xsp, ip)

    assert rc(xp=None) == BAD and b"null" in L.fl_last_error()
    assert rc(wp=None) == BAD and rc(xsp=None) == BAD and rc(ip=None) == BAD
    assert rc(h=12) == BAD and b"multiple of 8" in L.fl_last_error()
    assert rc(T=0) == BAD and rc(T=-1) == BAD and rc(h=0) == BAD
    assert rc(n_slab=2) == BAD and b"n_slab" in L.fl_last_error()                           # slabs without a delta
    assert rc(dp=d.ctypes.data, n_slab=0) == BAD and rc(dp=d.ctypes.data, n_slab=65) == BAD and rc(n_slab=-1) == BAD
    assert rc(dtype=2) == UNSUPPORTED                                                       # fp16
    assert (x == 1).all() and (xs == 0).all() and (inv == 0).all()                          # a refused call writes nothing
    assert rc(dp=d.ctypes.data, n_slab=3) in (0, NO_DEVICE)                                 # well-formed: the device, or the loud "no device"


def _norm_args(fa, form=0, T=1, N=32, K=64, dtype=1, epilogue=0, pro=1, n_slab=0, repeat=1, embed=False, bias=False, w_scale=True):
    b = fa.binding
    Ta, Na, Ka = max(T, 1), max(N, 1), max(K, 8)                      # (the arrays of a call with a bad size are never read)
    keep = dict(x=np.ones((Ta, Ka), np.float32), d=np.ones((min(max(n_slab, 1), 8), Ta, Ka), np.float32), nw=np.ones(Ka, np.float32),
                w=np.zeros((Na, Ka), np.uint16 if dtype == 1 else np.float32), s=np.ones(Na, np.float32), bias=np.ones(Na, np.float32),
                y=np.full((Ta, Na), 7.0, np.float32), xo=np.full((Ta, Ka), 7.0, np.float32), k=np.zeros(4, np.int32),
                e=np.zeros((5, Ka), np.uint16 if dtype == 1 else np.float32), tok=np.full(Ta, 3, np.uint32), xb=np.zeros((Ta, Ka), np.uint16))
    a = b.FlNormLinearArgs()
    a.struct_size = C.sizeof(b.FlNormLinearArgs)
    a.form, a.dtype, a.epilogue, a.pro, a.T, a.N, a.K, a.n_slab, a.repeat, a.eps = form, dtype, epilogue, pro, T, N, K, n_slab, repeat, 1e-5
    a.norm_w, a.w, a.y, a.x_out, a.kernels_out = (keep[n].ctypes.data for n in ("nw", "w", "y", "xo", "k"))
    if embed:
        a.embed, a.tokens, a.vocab = keep["e"].ctypes.data, keep["tok"].ctypes.data, 5
    elif pro == 1:
        a.x_res = keep["x"].ctypes.data
    else:
        a.x = keep["xb"].ctypes.data
    if n_slab:
        a.delta = keep["d"].ctypes.data
    if bias:
        a.bias = keep["bias"].ctypes.data
    if w_scale:
        a.w_scale = keep["s"].ctypes.data
    return a, keep


def test_norm_linear_argument_errors(fa, L):
    def rc(edit=None, **kw):
        a, keep = _norm_args(fa, **kw)
        if edit:
            edit(a)
        r = L.fl_op_norm_linear(C.byref(a))
        if r in (BAD, UNSUPPORTED):
            assert (keep["y"] == 7).all() and (keep["xo"] == 7).all()                       # a refused call writes nothing
        return r

    def clear(*names):
        def edit(a):
            for n in names:
                setattr(a, n, None if n not in ("struct_size", "vocab") else 0)
        return edit

    assert L.fl_op_norm_linear(None) == BAD and b"null args" in L.fl_last_error()
    assert rc(clear("struct_size")) == BAD and b"struct_size" in L.fl_last_error()
    assert rc(form=4) == BAD and rc(form=-1) == BAD and b"form" in L.fl_last_error()
    assert rc(clear("w")) == BAD and rc(clear("y")) == BAD and rc(clear("norm_w")) == BAD and rc(clear("x_res")) == BAD
    assert rc(K=68) == BAD and b"multiple of 8" in L.fl_last_error()                         # h % 8
    assert rc(T=0) == BAD and rc(T=-3) == BAD and rc(N=0) == BAD
    assert rc(epilogue=1, N=33) == BAD and b"even" in L.fl_last_error()                      # odd N for gate/up
    assert rc(epilogue=1, bias=True) == BAD and rc(epilogue=2) == BAD
    assert rc(repeat=0) == BAD and rc(repeat=9) == BAD
    assert rc(n_slab=65) == BAD and rc(clear("delta"), n_slab=2) == BAD
    assert rc(pro=0) == BAD and b"form 3" in L.fl_last_error()                               # the plain form is the batched stream's
    assert rc(pro=0, form=3, edit=clear("x")) == BAD
    assert rc(embed=True, edit=clear("tokens")) == BAD and rc(embed=True, edit=clear("vocab")) == BAD
    assert rc(embed=True, edit=lambda a: setattr(a, "vocab", 3)) == BAD and b"not below vocab" in L.fl_last_error()
    assert rc(dtype=2) == UNSUPPORTED
    # the forms' own limits
    assert rc(form=1, T=2) == BAD and rc(form=2, T=2) == BAD
    assert rc(form=1, K=6152) == UNSUPPORTED and b"6144" in L.fl_last_error()
    assert rc(form=1, K=6152, dtype=0) == UNSUPPORTED
    assert rc(form=2, K=6160) == UNSUPPORTED and rc(form=2, K=72) == UNSUPPORTED             # K % 16
    assert rc(form=2, dtype=0) == UNSUPPORTED and rc(form=2, n_slab=2) == UNSUPPORTED
    assert rc(form=2, w_scale=False) == BAD
    assert rc(form=3, T=9) == BAD and b"at most 8" in L.fl_last_error()                      # B > 8
    assert rc(form=3, T=4, dtype=0) == UNSUPPORTED
    for form, T in ((0, 5), (1, 1), (2, 1), (3, 8)):
        assert rc(form=form, T=T) in (0, NO_DEVICE), form                                    # well-formed: the device, or the loud "no device"


def test_linear_resid_argument_errors(fa, L):
    b = fa.binding
    T, N, K, N2 = 4, 16, 64, 32
    keep = dict(x=np.zeros((T, K), np.uint16), w=np.zeros((N, K), np.uint16), h=np.ones((T, N), np.float32), wn=np.ones(N, np.float32),
                w2=np.zeros((N2, N), np.uint16), ho=np.full((T, N), 7.0, np.float32), xn=np.zeros((T, N), np.float32), inv=np.zeros(T, np.float32),
                part=np.zeros((T, 4), np.float32), y2=np.zeros((T, N2), np.float32), k=np.zeros(6, np.int32))

    def rc(edit=None):
        a = b.FlLinearResidArgs()
        a.struct_size = C.sizeof(b.FlLinearResidArgs)
        a.T, a.N, a.K, a.N2, a.eps, a.lazy, a.epi2, a.repeat = T, N, K, 0, 1e-5, 0, 0, 1
        a.x, a.w, a.h_in, a.w_next, a.h_out, a.xn_out, a.inv_rms_out, a.part_out, a.kernels_out = (
            keep[n].ctypes.data for n in ("x", "w", "h", "wn", "ho", "xn", "inv", "part", "k"))
        if edit:
            edit(a)
        r = L.fl_op_linear_resid(C.byref(a))
        assert (keep["ho"] == 7).all() or r == 0
        return r

    def put(**kw):
        def edit(a):
            for n, v in kw.items():
                setattr(a, n, v)
        return edit

    assert L.fl_op_linear_resid(None) == BAD and b"null args" in L.fl_last_error()
    assert rc(put(struct_size=8)) == BAD and b"struct_size" in L.fl_last_error()
    for name in ("x", "w", "h_in", "w_next", "h_out", "xn_out", "inv_rms_out", "part_out"):
        assert rc(put(**{name: None})) == BAD, name
    assert rc(put(T=0)) == BAD and rc(put(N=0)) == BAD and rc(put(K=-8)) == BAD
    assert rc(put(K=68)) == BAD and rc(put(N=12)) == BAD and b"multiples of 8" in L.fl_last_error()
    assert rc(put(repeat=0)) == BAD and rc(put(repeat=9)) == BAD
    w2, y2 = keep["w2"].ctypes.data, keep["y2"].ctypes.data
    assert rc(put(w2=w2, N2=N2)) == BAD and b"consumer" in L.fl_last_error()                 # no y2_out
    assert rc(put(w2=w2, y2_out=y2, N2=0)) == BAD and rc(put(w2=w2, y2_out=y2, N2=N2, epi2=2)) == BAD
    assert rc(put(w2=w2, y2_out=y2, N2=33, epi2=1)) == BAD                                   # odd N2 for gate/up
    # well-formed: no device here; on a GPU the planner's answer for four rows (by default: no kernel takes the residual epilogue)
    assert rc() in (0, NO_DEVICE, UNSUPPORTED)
