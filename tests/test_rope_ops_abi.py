"""The RoPE + KV-append op entry points without a GPU: fl_op_rope_kv / fl_op_qkv_rope are exported and declared, their argument structs
have the header's layout, and their argument errors come back before the device is touched."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "fastllm_mi355x.h")
NEW = ("fl_op_rope_kv", "fl_op_qkv_rope")
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
    """every field of the three ctypes mirrors at the header's offset"""
    b = fa.binding
    lines = ['#include <stddef.h>', '#include "%s"' % HEADER]
    for cname, st in (("fl_rope_seqs", b.FlRopeSeqs), ("fl_rope_kv_args", b.FlRopeKvArgs), ("fl_qkv_rope_args", b.FlQkvRopeArgs)):
        lines.append('_Static_assert(sizeof(%s) == %d, "sizeof(%s)");' % (cname, C.sizeof(st), cname))
        for name, _ in st._fields_:
            lines.append('_Static_assert(offsetof(%s, %s) == %d, "%s.%s");' % (cname, name, getattr(st, name).offset, cname, name))
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "layout.c")
        open(c, "w").write("\n".join(lines) + "\nint main(void) { return 0; }\n")
        r = subprocess.run(["gcc", "-std=c11", "-fsyntax-only", c], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr


class Seqs:
    """an fl_rope_seqs over arrays this object keeps alive; caches full of 7"""

    def __init__(self, st, counts, pos, lens, sa, vt, layers, layer, Hkv, d, bf16):
        n = len(counts)
        self.cols = [np.array(c, dtype=np.int32) for c in (counts, pos, lens, sa, vt)]
        et = np.uint16 if bf16 else np.float32
        self.k = [np.full(max(layers, 1) * Hkv * max(s, 1) * max(d, 1), 7, et) for s in sa]
        self.v = [np.full(max(layers, 1) * Hkv * max(s, 1) * max(d, 1), 7, et) for s in sa]
        self.kp = (C.c_void_p * n)(*[a.ctypes.data for a in self.k])
        self.vp = (C.c_void_p * n)(*[a.ctypes.data for a in self.v])
        st.n_seq, st.layers, st.layer = n, layers, layer
        st.count, st.pos, st.len, st.seq_alloc, st.v_transposed = (c.ctypes.data for c in self.cols)
        st.k_cache, st.v_cache = C.addressof(self.kp), C.addressof(self.vp)

    def untouched(self):
        return all((a == 7).all() for a in self.k + self.v)


def _seq_kw(kw, T):
    n = kw.pop("n_seq", 1)
    return dict(counts=kw.pop("counts", [T] if n == 1 else [1] * n), pos=kw.pop("pos", [0] * n), lens=kw.pop("lens", [0] * n),
                sa=kw.pop("sa", [32] * n), vt=kw.pop("vt", [0] * n), layers=kw.pop("layers", 1), layer=kw.pop("layer", 0))


def _rope_kv_args(fa, form=0, dtype=1, H=2, Hkv=1, d=8, max_pos=16, n_slab=1, repeat=1, rows=3, bias=False, **kw):
    b = fa.binding
    N = (H + 2 * Hkv) * max(d, 2)
    keep = dict(qkv=np.ones((min(max(n_slab, 1), 8), rows, N), np.float32), bias=np.ones(N, np.float32), cos=np.ones((max(max_pos, 1), max(d, 2) // 2), np.float32),
                sin=np.zeros((max(max_pos, 1), max(d, 2) // 2), np.float32), q=np.full((rows, H * max(d, 2)), 7, np.uint16 if dtype == 1 else np.float32),
                k=np.zeros(4, np.int32))
    a = b.FlRopeKvArgs()
    a.struct_size = C.sizeof(b.FlRopeKvArgs)
    a.form, a.dtype, a.n_slab, a.repeat, a.H, a.Hkv, a.d, a.max_pos = form, dtype, n_slab, repeat, H, Hkv, d, max_pos
    a.qkv, a.cos_tab, a.sin_tab, a.q_out, a.kernels_out = (keep[n].ctypes.data for n in ("qkv", "cos", "sin", "q", "k"))
    if bias:
        a.bias = keep["bias"].ctypes.data
    keep["seqs"] = Seqs(a.seqs, Hkv=Hkv, d=d, bf16=dtype == 1, **_seq_kw(kw, rows))
    assert not kw, kw
    return a, keep


def _edit(**kw):
    def edit(a):
        for n, v in kw.items():
            obj = a.seqs if n in ("count", "pos", "len", "seq_alloc", "v_transposed", "k_cache", "v_cache") else a
            setattr(obj, n, v)
    return edit


def test_rope_kv_argument_errors(fa, L):
    def rc(edit=None, **kw):
        a, keep = _rope_kv_args(fa, **kw)
        if edit:
            edit(a)
        r = L.fl_op_rope_kv(C.byref(a))
        if r in (BAD, UNSUPPORTED):
            assert (keep["q"] == 7).all() and keep["seqs"].untouched() and (keep["k"] == 0).all()       # a refused call writes nothing
        return r

    assert L.fl_op_rope_kv(None) == BAD and b"null args" in L.fl_last_error()
    assert rc(_edit(struct_size=8)) == BAD and b"struct_size" in L.fl_last_error()
    assert rc(form=3) == BAD and rc(form=-1) == BAD and b"form" in L.fl_last_error()
    for name in ("qkv", "cos_tab", "sin_tab", "q_out", "count", "pos", "len", "seq_alloc", "v_transposed", "k_cache", "v_cache"):
        assert rc(_edit(**{name: None})) == BAD, name
    assert rc(n_slab=0) == BAD and rc(n_slab=65) == BAD and rc(repeat=0) == BAD and rc(repeat=9) == BAD
    assert rc(dtype=2) == UNSUPPORTED
    # the errors both entry points share
    assert rc(lens=[30]) == BAD and b"exceeds seq_alloc" in L.fl_last_error()                  # 30 + 3 > 32
    assert rc(lens=[29]) in (0, NO_DEVICE)                                                     # ... and len + count == seq_alloc is allowed
    assert rc(pos=[14]) == BAD and b"exceeds max_pos" in L.fl_last_error()                     # 14 + 3 > 16
    assert rc(pos=[13]) in (0, NO_DEVICE)
    assert rc(d=7) == BAD and b"even" in L.fl_last_error()
    assert rc(H=3, Hkv=2) == BAD and b"multiple of Hkv" in L.fl_last_error()
    assert rc(layers=2, layer=2) == BAD and b"layer" in L.fl_last_error()
    assert rc(layers=0) == BAD and rc(layer=-1) == BAD
    assert rc(counts=[0]) == BAD and rc(pos=[-1]) == BAD and rc(lens=[-1]) == BAD and rc(max_pos=0) == BAD
    # what each form cannot take
    assert rc(form=0, n_seq=2, rows=2) == BAD and b"one sequence" in L.fl_last_error()
    assert rc(form=1, n_seq=2, rows=3, counts=[1, 2]) == BAD and b"one row per sequence" in L.fl_last_error()
    assert rc(form=1, n_seq=2, rows=2, vt=[1, 0]) == UNSUPPORTED and b"one value layout" in L.fl_last_error()
    assert rc(form=1, n_seq=2, rows=2, vt=[1, 1], dtype=0) == UNSUPPORTED and b"row-major" in L.fl_last_error()
    for form, kw in ((0, {}), (1, dict(n_seq=3, rows=3)), (2, dict(n_seq=2, rows=3, counts=[1, 2], vt=[1, 0]))):
        assert rc(form=form, **kw) in (0, NO_DEVICE), form                                     # well-formed: the device, or the loud "no device"


def _qkv_rope_args(fa, form=0, dtype=1, T=1, K=64, H=2, Hkv=1, d=8, max_pos=16, n_slab=0, repeat=1, embed=False, bias=False, w_scale=True, **kw):
    b = fa.binding
    N, Ta, Ka = (H + 2 * Hkv) * max(d, 2), max(T, 1), max(K, 8)
    et = np.uint16 if dtype == 1 else np.float32
    keep = dict(x=np.ones((Ta, Ka), np.float32), dl=np.ones((min(max(n_slab, 1), 8), Ta, Ka), np.float32), nw=np.ones(Ka, np.float32), w=np.zeros((N, Ka), et),
                s=np.ones(N, np.float32), bias=np.ones(N, np.float32), cos=np.ones((max(max_pos, 1), max(d, 2) // 2), np.float32),
                sin=np.zeros((max(max_pos, 1), max(d, 2) // 2), np.float32), q=np.full((Ta, H * max(d, 2)), 7, et), xo=np.full((Ta, Ka), 7.0, np.float32),
                k=np.zeros(4, np.int32), e=np.zeros((5, Ka), et), tok=np.full(Ta, 3, np.uint32))
    a = b.FlQkvRopeArgs()
    a.struct_size = C.sizeof(b.FlQkvRopeArgs)
    a.form, a.dtype, a.n_slab, a.repeat, a.T, a.K, a.H, a.Hkv, a.d, a.max_pos, a.eps = form, dtype, n_slab, repeat, T, K, H, Hkv, d, max_pos, 1e-5
    a.norm_w, a.w, a.cos_tab, a.sin_tab, a.q_out, a.x_out, a.kernels_out = (keep[n].ctypes.data for n in ("nw", "w", "cos", "sin", "q", "xo", "k"))
    if embed:
        a.embed, a.tokens, a.vocab = keep["e"].ctypes.data, keep["tok"].ctypes.data, 5
    else:
        a.x_res = keep["x"].ctypes.data
    if n_slab:
        a.delta = keep["dl"].ctypes.data
    if bias:
        a.bias = keep["bias"].ctypes.data
    if w_scale:
        a.w_scale = keep["s"].ctypes.data
    if form == 3:
        kw.setdefault("n_seq", Ta)
        kw.setdefault("vt", [1] * kw["n_seq"])
    keep["seqs"] = Seqs(a.seqs, Hkv=Hkv, d=d, bf16=dtype == 1, **_seq_kw(kw, Ta))
    assert not kw, kw
    return a, keep


def test_qkv_rope_argument_errors(fa, L):
    def rc(edit=None, **kw):
        a, keep = _qkv_rope_args(fa, **kw)
        if edit:
            edit(a)
        r = L.fl_op_qkv_rope(C.byref(a))
        if r in (BAD, UNSUPPORTED):
            assert (keep["q"] == 7).all() and (keep["xo"] == 7).all() and keep["seqs"].untouched() and (keep["k"] == 0).all()
        return r

    assert L.fl_op_qkv_rope(None) == BAD and b"null args" in L.fl_last_error()
    assert rc(_edit(struct_size=8)) == BAD and b"struct_size" in L.fl_last_error()
    assert rc(form=4) == BAD and rc(form=-1) == BAD and b"form" in L.fl_last_error()
    for name in ("w", "norm_w", "x_res", "cos_tab", "sin_tab", "q_out", "count", "pos", "len", "seq_alloc", "v_transposed", "k_cache", "v_cache"):
        assert rc(_edit(**{name: None})) == BAD, name
    assert rc(K=68) == BAD and b"multiple of 8" in L.fl_last_error()
    assert rc(T=0) == BAD and rc(K=0) == BAD and rc(repeat=0) == BAD and rc(repeat=9) == BAD
    assert rc(n_slab=65) == BAD and rc(_edit(delta=None), n_slab=2) == BAD
    assert rc(embed=True, edit=_edit(tokens=None)) == BAD and rc(embed=True, edit=_edit(vocab=3)) == BAD and b"not below vocab" in L.fl_last_error()
    assert rc(dtype=2) == UNSUPPORTED
    # the errors both entry points share
    assert rc(T=3, lens=[30]) == BAD and b"exceeds seq_alloc" in L.fl_last_error()
    assert rc(T=3, pos=[14]) == BAD and b"exceeds max_pos" in L.fl_last_error()
    assert rc(d=7) == BAD and b"even" in L.fl_last_error()
    assert rc(H=3, Hkv=2) == BAD and b"multiple of Hkv" in L.fl_last_error()
    assert rc(layers=2, layer=2) == BAD and b"layer" in L.fl_last_error()
    assert rc(T=3, counts=[2]) == BAD and b"rows" in L.fl_last_error()                        # the counts do not add up to T
    # what each form cannot take
    assert rc(form=0, T=2, n_seq=2) == BAD and b"one sequence" in L.fl_last_error()
    assert rc(form=1, T=2) == BAD and rc(form=2, T=2) == BAD
    assert rc(form=1, K=6152) == UNSUPPORTED and b"6144" in L.fl_last_error()
    assert rc(form=2, K=6160) == UNSUPPORTED and rc(form=2, K=72) == UNSUPPORTED             # K % 16
    assert rc(form=2, dtype=0) == UNSUPPORTED and rc(form=2, n_slab=2) == UNSUPPORTED
    assert rc(form=2, w_scale=False) == BAD
    assert rc(form=3, T=9) == BAD and b"at most 8" in L.fl_last_error()
    assert rc(form=3, T=4, n_seq=2, counts=[2, 2]) == BAD and b"one sequence per row" in L.fl_last_error()
    assert rc(form=3, T=4, dtype=0) == UNSUPPORTED
    assert rc(form=3, T=2, vt=[1, 0]) == UNSUPPORTED and b"transposed" in L.fl_last_error()
    assert rc(form=3, T=8, K=16384) == UNSUPPORTED and b"K slices" in L.fl_last_error()
    for form, T in ((0, 5), (1, 1), (2, 1), (3, 8)):
        assert rc(form=form, T=T) in (0, NO_DEVICE), form                                    # well-formed: the device, or the loud "no device"
