"""fl_op_attn_oproj_rep without a GPU: the symbol is exported and declared, its argument struct has the header's layout, argument
errors come back before the device is touched and write nothing, and -- through query_only -- the table of what the launch takes:
where the model's capacity rule flips, which head shapes are refused, rows per wave and GMAX."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "fastllm_mi355x.h")
BAD, NO_DEVICE, UNSUPPORTED = -8, -9, -10


@pytest.fixture(scope="module")
def fa():
    import fastllm_amd
    return fastllm_amd


@pytest.fixture(scope="module")
def L(fa):
    return fa.lib()


def test_symbol_is_exported_and_declared(fa, L):
    hdr = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert hasattr(L, "fl_op_attn_oproj_rep")
    assert re.search(r"\bfl_op_attn_oproj_rep\s*\(", hdr)
    out = subprocess.check_output(["nm", "-D", "--defined-only", fa.binding.LIB_PATH], text=True)
    assert "fl_op_attn_oproj_rep" in set(re.findall(r" T (fl_[a-z_0-9]+)", out))
    assert re.search(r"#define\s+FL_ABI_VERSION\s+2\b", hdr) and L.fl_abi_version() == 2      # the change only adds an entry


def test_argument_struct_has_the_header_layout(fa):
    st = fa.binding.FlAttnOprojRepArgs
    lines = ['#include <stddef.h>', '#include "%s"' % HEADER,
             '_Static_assert(sizeof(fl_attn_oproj_rep_args) == %d, "sizeof(fl_attn_oproj_rep_args)");' % C.sizeof(st)]
    for name, _ in st._fields_:
        lines.append('_Static_assert(offsetof(fl_attn_oproj_rep_args, %s) == %d, "fl_attn_oproj_rep_args.%s");' % (name, getattr(st, name).offset, name))
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "layout.c")
        open(c, "w").write("\n".join(lines) + "\nint main(void) { return 0; }\n")
        r = subprocess.run(["gcc", "-std=c11", "-fsyntax-only", c], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr


def _args(fa, H=4, Hkv=2, d=64, N=9, s_past=2, k_rows=5, capacity=40, pad=0.0, repeat=2, query_only=0):
    st = fa.binding.FlAttnOprojRepArgs
    Ka, da = max(H, 1) * max(d, 1), max(d, 1)
    keep = dict(q=np.zeros(Ka, np.uint16), k=np.zeros((max(k_rows, 1), max(Hkv, 1) * da), np.uint16), v=np.zeros((max(k_rows, 1), max(Hkv, 1) * da), np.uint16),
                w=np.zeros((max(N, 1), Ka), np.uint16), out=np.full((16, max(N, 1)), 7.0, np.float32), info=np.full(6, -7, np.int32))
    a = st()
    a.struct_size = C.sizeof(st)
    a.H, a.Hkv, a.d, a.N, a.s_past, a.k_rows, a.capacity, a.pad_value, a.repeat, a.query_only = H, Hkv, d, N, s_past, k_rows, capacity, pad, repeat, query_only
    a.q, a.k, a.v, a.w_o, a.out, a.info_out = (keep[n].ctypes.data for n in ("q", "k", "v", "w", "out", "info"))
    return a, keep


def test_argument_errors_write_nothing(fa, L):
    def rc(edit=None, **kw):
        a, keep = _args(fa, **kw)
        for n, v in (edit or {}).items():
            setattr(a, n, v)
        r = L.fl_op_attn_oproj_rep(C.byref(a))
        if r in (BAD, UNSUPPORTED):
            assert (keep["out"] == 7).all() and (keep["info"] == -7).all()                      # a refused call writes nothing
        return r

    assert L.fl_op_attn_oproj_rep(None) == BAD and b"null args" in L.fl_last_error()
    assert rc(dict(struct_size=8)) == BAD and b"struct_size" in L.fl_last_error()
    for name in ("q", "k", "v", "w_o", "out"):
        assert rc({name: None}) == BAD, name
    assert rc(dict(info_out=None)) in (0, NO_DEVICE)                                            # optional ...
    assert rc(dict(info_out=None), query_only=1) == BAD                                         # ... but all a query writes
    assert rc(query_only=2) == BAD and rc(query_only=-1) == BAD
    assert rc(H=0) == BAD and rc(Hkv=0) == BAD and rc(H=5, Hkv=2) == BAD and b"multiple of Hkv" in L.fl_last_error()
    assert rc(d=0) == BAD and rc(N=0) == BAD and rc(N=(1 << 20) + 1) == BAD and rc(capacity=0) == BAD
    assert rc(s_past=-1) == BAD and rc(s_past=5) == BAD and b"k_rows" in L.fl_last_error()      # S = 6 > k_rows = 5
    assert rc(s_past=4) in (0, NO_DEVICE)                                                       # S == k_rows is allowed
    assert rc(k_rows=41) == BAD and rc(k_rows=40) in (0, NO_DEVICE)                             # k_rows <= capacity
    assert rc(pad=float("nan")) == BAD and rc(pad=float("inf")) == BAD and b"finite" in L.fl_last_error()
    assert rc(repeat=0) == BAD and rc(repeat=17) == BAD and rc(repeat=16) in (0, NO_DEVICE)
    # head shapes the kernel does not take: with and without query_only
    for q in (0, 1):
        assert rc(H=9, Hkv=1, query_only=q) == UNSUPPORTED                                      # G = 9
        assert rc(H=6, Hkv=3, query_only=q) == UNSUPPORTED                                      # 8 % Hkv
        assert rc(d=96, query_only=q) == UNSUPPORTED and b"head shape" in L.fl_last_error()
        assert rc(H=33, Hkv=33, query_only=q) == UNSUPPORTED                                    # K = 2112 > 2048 (and 8 % 33)
        assert rc(H=16, Hkv=4, d=128, query_only=q) in (0, NO_DEVICE)                           # K = 2048 is taken
    # more than 32 key tiles per slice: the op refuses to run it, a query reports it
    assert rc(H=8, Hkv=8, capacity=32 * 33, k_rows=5) == UNSUPPORTED and b"32 key tiles" in L.fl_last_error()
    assert rc(H=8, Hkv=8, capacity=32 * 32, k_rows=5) in (0, NO_DEVICE)
    assert rc(H=8, Hkv=8, capacity=32 * 33, query_only=1) == 0
    assert rc() in (0, NO_DEVICE)                                                               # well-formed: the device, or the loud "no device"


def test_query_only_needs_no_device_and_no_operands(fa):
    info = fa.op_attn_oproj_rep_info(4, 2, 64, 9, 40)
    assert list(info) == [1, 1, 1, 4, 2, 4]                                                     # 9 rows over 8 waves: 2 workgroups; nslice 8 / 2


def test_model_rule_flips_at_96_KiB(fa):
    """Hkv * sa * d = 24576 (2 bytes, K and V: 96 KiB) is the last allocation the decode step takes"""
    for Hkv, d, yes, no in ((1, 64, 384, 416), (2, 64, 192, 224), (4, 64, 96, 128), (8, 64, 32, 64), (1, 128, 192, 224), (4, 128, 32, 64)):
        H = Hkv * 2
        for sa, want in ((yes, 1), (no, 0)):
            for cap in (sa - 31, sa):                                                           # the capacity is rounded up to 32 rows
                info = fa.op_attn_oproj_rep_info(H, Hkv, d, 64, cap)
                assert info[0] == want and info[1] == 1, (Hkv, d, cap, list(info))
        assert (Hkv * yes * d <= 24576) and (Hkv * no * d > 24576)
    info = fa.op_attn_oproj_rep_info(8, 8, 128, 64, 32)                                         # one tile of it is 128 KiB already
    assert info[0] == 0 and info[1] == 1
    # the any-size rule: 32 tiles per slice
    assert fa.op_attn_oproj_rep_info(8, 1, 64, 64, 32 * 8 * 32)[1] == 1 and fa.op_attn_oproj_rep_info(8, 1, 64, 64, 32 * 8 * 32 + 1)[1] == 0
    assert fa.op_attn_oproj_rep_info(8, 8, 64, 64, 32 * 32)[1] == 1 and fa.op_attn_oproj_rep_info(8, 8, 64, 64, 32 * 32 + 1)[1] == 0


def test_refused_head_shapes(fa):
    # G = 9; 8 % Hkv; d; K = 2112 (which no head count reaches without also breaking G or Hkv); K = 2560 and 3072 with nothing else wrong
    for H, Hkv, d in ((9, 1, 64), (18, 2, 64), (3, 3, 64), (6, 3, 128), (4, 2, 96), (33, 1, 64), (40, 8, 64), (24, 4, 128)):
        with pytest.raises(fa.FastLLMError) as e:
            fa.op_attn_oproj_rep_info(H, Hkv, d, 64, 32)
        assert e.value.code == UNSUPPORTED, (H, Hkv, d)
    assert fa.op_attn_oproj_rep_info(32, 4, 64, 64, 32)[0] == 1                                 # K = 2048, G = 8


def test_rows_per_wave_gmax_workgroups_and_slices(fa):
    for N, rpw, blocks in ((1, 1, 1), (8, 1, 1), (9, 1, 2), (2048, 1, 256), (2049, 2, 129), (2048 + 17, 2, 130), (4096, 2, 256)):
        info = fa.op_attn_oproj_rep_info(8, 2, 64, N, 64)
        assert (info[2], info[4]) == (rpw, blocks), (N, list(info))
    for H, Hkv, gmax in ((8, 8, 4), (8, 4, 4), (6, 2, 4), (4, 1, 4), (5, 1, 8), (16, 2, 8), (8, 1, 8)):            # G = 1, 2, 3, 4 -> 4; 5, 8 -> 8
        for d in (64, 128):
            info = fa.op_attn_oproj_rep_info(H, Hkv, d, 64, 32)
            assert info[3] == gmax and info[5] == 8 // Hkv, (H, Hkv, d, list(info))
