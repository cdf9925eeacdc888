"""fl_op_convert_slice and fl_op_model_tensor without a GPU: the symbols are exported and declared, fl_convert_slice_args has the
header's layout, every argument error comes back before the device is touched (and writes nothing), and a well-formed call fails
loudly where there is no GPU."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "fastllm_mi355x.h")
BAD, NO_DEVICE = -8, -9
NEW = ("fl_op_convert_slice", "fl_op_model_tensor")


@pytest.fixture(scope="module")
def fa():
    import fastllm_amd
    return fastllm_amd


@pytest.fixture(scope="module")
def L(fa):
    return fa.lib()


def _header():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def test_symbols_are_exported_and_declared(fa, L):
    hdr = _header()
    out = subprocess.check_output(["nm", "-D", "--defined-only", fa.binding.LIB_PATH], text=True)
    for name in NEW:
        assert hasattr(L, name) and re.search(r"\b%s\s*\(" % name, hdr), name
        assert " T %s\n" % name in out, name
    assert re.search(r"#define\s+FL_ABI_VERSION\s+2\b", hdr) and L.fl_abi_version() == 2      # the change only adds entries
    # the selector names of the binding are the header's FL_MT_* values, and the e4m3 element code is next to the fl_dtype ones
    c_vals = dict((k, int(v)) for k, v in re.findall(r"\bFL_MT_([A-Z0-9_]+)\s*=\s*(\d+)", hdr))
    assert len(c_vals) == 22 and {k.lower(): v for k, v in c_vals.items()} == fa.MODEL_TENSORS
    assert re.search(r"\bFL_ELEM_E4M3\s*=\s*3\b", hdr) and fa.ELEM_E4M3 == 3 and (fa.binding.F32, fa.binding.BF16, fa.binding.F16) == (0, 1, 2)


def test_argument_struct_has_the_header_layout(fa, tmp_path):
    S = fa.FlConvertSliceArgs
    lines = ["#include <stddef.h>", '#include "%s"' % HEADER, '_Static_assert(sizeof(fl_convert_slice_args) == %d, "sizeof");' % C.sizeof(S)]
    for name, _ in S._fields_:
        lines.append('_Static_assert(offsetof(fl_convert_slice_args, %s) == %d, "%s");' % (name, getattr(S, name).offset, name))
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines) + "\nint main(void) { return 0; }\n")
    r = subprocess.run(["gcc", "-std=c11", "-fsyntax-only", str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    body = re.search(r"typedef struct fl_convert_slice_args \{(.*?)\} fl_convert_slice_args;", _header(), re.S).group(1)
    n_c = sum(len(decl.split(",")) for decl in body.split(";") if decl.strip())
    assert n_c == len(S._fields_)                            # no field of the header is missing from the mirror


def _args(fa, src_dtype=0, dst_dtype=1, R=40, Cc=24, r0=3, c0=8, rows=20, cols=16, dst_rows=48, dst_ld=64, dst_row0=0, row_mode=0, head_pad=0,
          dm=0, d=0):
    """a call over small arrays this function keeps alive; the destination full of 7"""
    keep = dict(src=np.zeros((max(R, 1), max(Cc, 1)), np.float32 if src_dtype == 0 else np.uint16),
                dst=np.full((max(dst_rows, 1), max(dst_ld, 1)), 7, np.uint32))
    a = fa.FlConvertSliceArgs()
    a.struct_size = C.sizeof(fa.FlConvertSliceArgs)
    a.src_dtype, a.dst_dtype, a.row_mode, a.head_pad = src_dtype, dst_dtype, row_mode, head_pad
    a.R, a.C, a.r0, a.c0, a.rows, a.cols, a.dst_rows, a.dst_ld, a.dst_row0, a.dm, a.d = R, Cc, r0, c0, rows, cols, dst_rows, dst_ld, dst_row0, dm, d
    a.src, a.dst = keep["src"].ctypes.data, keep["dst"].ctypes.data
    return a, keep


def test_convert_slice_argument_errors_come_before_the_device(fa, L):
    def rc(edit=None, **kw):
        a, keep = _args(fa, **kw)
        for n, v in (edit or {}).items():
            setattr(a, n, v)
        r = L.fl_op_convert_slice(C.byref(a))
        if r == BAD:
            assert (keep["dst"] == 7).all()                                                    # a refused call writes nothing
        return r

    assert L.fl_op_convert_slice(None) == BAD and b"null args" in L.fl_last_error()
    assert rc(dict(struct_size=8)) == BAD and b"struct_size" in L.fl_last_error()
    assert rc(dict(src=None)) == BAD and rc(dict(dst=None)) == BAD
    assert rc(src_dtype=3) == BAD and rc(src_dtype=-1) == BAD and b"src_dtype" in L.fl_last_error()
    assert rc(dst_dtype=2) == BAD and rc(dst_dtype=-1) == BAD and b"dst_dtype" in L.fl_last_error()        # no f16 destination
    assert rc(row_mode=3) == BAD and rc(row_mode=-1) == BAD and rc(head_pad=3) == BAD and rc(head_pad=-1) == BAD
    assert rc(dict(via_bf16=2)) == BAD and rc(dict(via_bf16=-1)) == BAD and rc(dict(via_bf16=1)) == BAD and b"via_bf16" in L.fl_last_error()   # (bf16 destination)
    assert rc(dict(via_bf16=1), dst_dtype=0) in (0, NO_DEVICE)
    assert rc(R=0) == BAD and rc(Cc=0) == BAD and rc(dst_rows=0) == BAD and rc(dst_ld=0) == BAD
    assert rc(dict(R=1 << 14, C=(1 << 12) + 1)) == BAD and rc(dict(dst_rows=1 << 14, dst_ld=(1 << 12) + 1)) == BAD      # above 2^26 elements
    assert rc(dict(R=1 << 40, C=1 << 40)) == BAD
    # the slice must stay in the source
    for kw in (dict(r0=-1), dict(c0=-1), dict(rows=0), dict(cols=0), dict(r0=21), dict(c0=9), dict(rows=38), dict(cols=17), dict(r0=1 << 62),
               dict(rows=1 << 62), dict(cols=1 << 62)):
        assert rc(**kw) == BAD, kw
    assert b"leaves the source" in L.fl_last_error()
    # every write must stay in the destination: the last row, the last column, the offset
    assert rc(dst_rows=19) == BAD and b"would land in row" in L.fl_last_error()
    assert rc(dst_ld=15) == BAD and b"would land in column" in L.fl_last_error()
    assert rc(dst_row0=29) == BAD and rc(dst_row0=-1) == BAD and rc(dst_row0=48) == BAD
    assert rc(dst_row0=28) in (0, NO_DEVICE)                                                   # rows 28 .. 47 of 48
    # the interleave: 20 rows reach row 32 + 3 (gate) and 32 + 16 + 3 (up); 16 rows end at 15 and at 31
    assert rc(row_mode=1, dst_rows=35) == BAD and rc(row_mode=1, dst_rows=36) in (0, NO_DEVICE)
    assert rc(row_mode=2, dst_rows=51) == BAD and rc(row_mode=2, dst_rows=52) in (0, NO_DEVICE)
    assert rc(row_mode=1, rows=16, dst_rows=15) == BAD and rc(row_mode=2, rows=16, dst_rows=31) == BAD
    assert rc(row_mode=2, rows=16, dst_rows=32) in (0, NO_DEVICE)
    assert rc(row_mode=1, dst_row0=1) == BAD and rc(row_mode=2, head_pad=1, dm=4, d=8) == BAD and b"interleave" in L.fl_last_error()
    # padded heads: 20 rows of dm 4 in d 8 are 5 heads, the last element at 4 * 8 + 4 + 1 = 37; 16 columns of dm 8 in d 64 end at 64 + 35
    assert rc(head_pad=1, dm=4, d=8, dst_rows=37) == BAD and rc(head_pad=1, dm=4, d=8, dst_rows=38) in (0, NO_DEVICE)
    assert rc(head_pad=1, dm=4, d=8, dst_rows=48, dst_row0=11) == BAD and rc(head_pad=1, dm=4, d=8, dst_rows=48, dst_row0=10) in (0, NO_DEVICE)
    assert rc(head_pad=2, dm=8, d=64, dst_ld=99) == BAD and rc(head_pad=2, dm=8, d=64, dst_ld=100) in (0, NO_DEVICE)
    for kw in (dict(dm=0, d=8), dict(dm=3, d=8), dict(dm=4, d=7), dict(dm=16, d=8), dict(dm=-2, d=8), dict(dm=2, d=(1 << 20) + 2)):
        assert rc(head_pad=1, **kw) == BAD and rc(head_pad=2, **kw) == BAD, kw
    assert b"head_pad" in L.fl_last_error()
    assert rc(dm=-5, d=-9) in (0, NO_DEVICE)                                                   # not looked at without head_pad
    for src_dtype in (0, 1, 2):                                                                # well-formed: the device, or the loud "no device"
        for dst_dtype in (0, 1):
            assert rc(src_dtype=src_dtype, dst_dtype=dst_dtype) in (0, NO_DEVICE)


def test_model_tensor_argument_errors_come_before_the_device(L):
    r, c, e = C.c_int64(-5), C.c_int64(-5), C.c_int32(-5)
    assert L.fl_op_model_tensor(None, 0, 0, 0, None, C.byref(r), C.byref(c), C.byref(e)) == BAD and b"null argument" in L.fl_last_error()
    assert (r.value, c.value, e.value) == (-5, -5, -5)


def test_no_cpu_path(fa):
    """Without a GPU the conversion fails loudly; nothing is computed on the host."""
    if fa.device_count() > 0:
        pytest.skip("a GPU is visible here")
    with pytest.raises(fa.FastLLMError) as e:
        fa.op_convert_slice(np.ones((4, 8), np.float32), 0, 0, 4, 8, "bf16", 4, 8)
    assert e.value.code == NO_DEVICE and "no CPU path" in str(e.value)
