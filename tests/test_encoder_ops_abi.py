"""fl_op_encoder_rows without a GPU: the symbol is exported and declared, fl_encoder_rows_args has the header's layout, every argument
error comes back before the device is touched (and writes nothing), and a well-formed call fails loudly where there is no GPU."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "fastllm_mi355x.h")
BAD, OVERFLOW, NO_DEVICE = -8, -7, -9


@pytest.fixture(scope="module")
def fa():
    import fastllm_amd
    return fastllm_amd


@pytest.fixture(scope="module")
def L(fa):
    return fa.lib()


def test_symbol_is_exported_and_declared(fa, L):
    hdr = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert hasattr(L, "fl_op_encoder_rows") and re.search(r"\bfl_op_encoder_rows\s*\(", hdr)
    out = subprocess.check_output(["nm", "-D", "--defined-only", fa.binding.LIB_PATH], text=True)
    assert " T fl_op_encoder_rows\n" in out
    assert re.search(r"#define\s+FL_ABI_VERSION\s+2\b", hdr) and L.fl_abi_version() == 2      # the change only adds an entry
    assert (fa.ENC_ACT[None], fa.ENC_ACT["gelu_tanh"], fa.ENC_ACT["gelu_erf"]) == (-1, 0, 1)


def test_argument_struct_has_the_header_layout(fa, tmp_path):
    S = fa.FlEncoderRowsArgs
    lines = ["#include <stddef.h>", '#include "%s"' % HEADER, '_Static_assert(sizeof(fl_encoder_rows_args) == %d, "sizeof");' % C.sizeof(S)]
    for name, _ in S._fields_:
        lines.append('_Static_assert(offsetof(fl_encoder_rows_args, %s) == %d, "%s");' % (name, getattr(S, name).offset, name))
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines) + "\nint main(void) { return 0; }\n")
    r = subprocess.run(["gcc", "-std=c11", "-fsyntax-only", str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    hdr = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    body = re.search(r"typedef struct fl_encoder_rows_args \{(.*?)\} fl_encoder_rows_args;", hdr, re.S).group(1)
    n_c = sum(len(decl.split(",")) for decl in body.split(";") if decl.strip())
    assert n_c == len(S._fields_)                            # no field of the header is missing from the mirror


def _args(fa, form, dtype=1, T=3, h=16, n_slab=2, repeat=1, act=0, vocab=5, P=4, offsets=(0, 1, 3), ids=(0, 4, 2)):
    """a well-formed call of `form` over small arrays this function keeps alive; outputs full of 7"""
    et = np.uint16 if dtype == 1 else np.float32
    hh, ns = max(h, 8), min(max(n_slab, 1), 8)
    keep = dict(word=np.zeros((max(vocab, 1), hh), et), pos=np.zeros((max(P, 1), hh), et), tt0=np.zeros(hh, et), ids=np.array(ids, np.uint32),
                offsets=np.array(offsets, np.uint64), x=np.ones((max(T, 1), hh), np.float32), slabs=np.ones((ns, max(T, 1), hh), np.float32),
                bias=np.ones(hh, np.float32), ln_w=np.ones(hh, np.float32), ln_b=np.zeros(hh, np.float32),
                x_res_out=np.full((max(T, 1), hh), 7, np.float32), out=np.full((max(T, 1), hh), 7, np.float32))
    a = fa.FlEncoderRowsArgs()
    a.struct_size = C.sizeof(fa.FlEncoderRowsArgs)
    a.form, a.dtype, a.n_slab, a.repeat, a.act, a.T, a.h, a.vocab, a.P, a.n_seq, a.eps = form, dtype, n_slab, repeat, act, T, h, vocab, P, len(offsets) - 1, 1e-5
    for name in (("word", "pos", "tt0", "ids", "offsets", "ln_w", "ln_b", "x_res_out"), ("x", "slabs", "bias", "ln_w", "ln_b", "x_res_out"), ("slabs", "bias"),
                 ("x", "offsets"))[form] + ("out",):
        setattr(a, name, keep[name].ctypes.data)
    return a, keep


def test_argument_errors_come_before_the_device(fa, L):
    def rc(form, edit=None, **kw):
        a, keep = _args(fa, form, **kw)
        for n, v in (edit or {}).items():
            setattr(a, n, v)
        r = L.fl_op_encoder_rows(C.byref(a))
        if r in (BAD, OVERFLOW):
            assert (keep["out"] == 7).all() and (keep["x_res_out"] == 7).all()                  # a refused call writes nothing
        return r

    assert L.fl_op_encoder_rows(None) == BAD and b"null args" in L.fl_last_error()
    for form in range(4):
        assert rc(form, dict(struct_size=8)) == BAD and b"struct_size" in L.fl_last_error()
        assert rc(form, dict(out=None)) == BAD and rc(form, repeat=0) == BAD and rc(form, repeat=9) == BAD
        assert rc(form, dtype=2) == BAD and b"dtype" in L.fl_last_error()
        assert rc(form, h=0) == BAD
    assert rc(0, dict(form=4)) == BAD and rc(0, dict(form=-1)) == BAD and b"form" in L.fl_last_error()
    # null pointers, per form
    for form, names in ((0, ("word", "pos", "ids", "offsets", "ln_w", "ln_b", "x_res_out")), (1, ("x", "slabs", "ln_w", "ln_b", "x_res_out")),
                        (2, ("slabs",)), (3, ("x", "offsets"))):
        for name in names:
            assert rc(form, {name: None}) == BAD, (form, name)
    # the row width
    for form in (0, 1, 2):
        assert rc(form, h=12) == BAD and b"multiple of 8" in L.fl_last_error()
    assert rc(3, h=12) in (0, NO_DEVICE)                                                       # pooling takes any width
    # the slabs and the rows of forms 1 and 2
    for form in (1, 2):
        assert rc(form, n_slab=0) == BAD and rc(form, n_slab=9) == BAD and b"n_slab" in L.fl_last_error()
        assert rc(form, T=0) == BAD
    assert rc(2, act=2) == BAD and rc(2, act=-2) == BAD and b"act" in L.fl_last_error()
    # the offsets of forms 0 and 3 (encoder_check_offsets), the ids and the positions of form 0
    for form in (0, 3):
        assert rc(form, offsets=(1, 2, 3)) == BAD and b"offsets[0]" in L.fl_last_error()
        assert rc(form, offsets=(0, 2, 1), ids=(0, 1)) == BAD and b"decrease" in L.fl_last_error()
        assert rc(form, offsets=(0, 1, 1, 3)) == BAD and b"empty" in L.fl_last_error()
        assert rc(form, dict(n_seq=0)) == BAD
    assert rc(0, ids=(0, 5, 2)) == BAD and b"not below vocab" in L.fl_last_error()            # vocab is 5
    assert rc(0, P=1) == OVERFLOW and b"max_position_embeddings" in L.fl_last_error()         # the second sequence has 2 rows
    assert rc(0, P=2) in (0, NO_DEVICE)                                                        # ... and len == P is allowed
    assert rc(0, P=0) == BAD and rc(0, vocab=0) == BAD
    for form in range(4):                                                                      # well-formed: the device, or the loud "no device"
        for dtype in (0, 1):
            assert rc(form, dtype=dtype) in (0, NO_DEVICE), (form, dtype)


def test_no_cpu_path(fa):
    """Without a GPU every form fails loudly; nothing is computed on the host."""
    if fa.device_count() > 0:
        pytest.skip("a GPU is visible here")
    x = np.ones((3, 16), np.float32)
    w = np.ones(16, np.float32)
    calls = (lambda: fa.op_encoder_embed_ln(x, x, [0, 1, 2], [1, 2], w, w, 1e-12, "f32"), lambda: fa.op_encoder_add_ln(x, x[None], w, w, 1e-5, "bf16"),
             lambda: fa.op_encoder_bias_act(x[None], "bf16", bias=w, act="gelu_erf"), lambda: fa.op_encoder_pool_l2(x, [1, 2]))
    for call in calls:
        with pytest.raises(fa.FastLLMError) as e:
            call()
        assert e.value.code == NO_DEVICE and "no CPU path" in str(e.value)
