"""CPU tests of the encoder's C ABI (fl_encoder_*, fl_op_encoder_attention): exported symbols, the struct layout against the ctypes
mirror, every error that is decided before the device probe, and the loud failure without a GPU (there is no CPU path)."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import bert_ref

NEW = ["fl_encoder_create", "fl_encoder_release", "fl_encoder_hidden", "fl_encoder_embed", "fl_op_encoder_attention"]
CFG = bert_ref.CONFIGS["bert_a"]


@pytest.fixture(scope="module")
def fa():
    import fastllm_amd
    return fastllm_amd


def create(fa, cfg=None, dtype=1, **over):
    """fl_encoder_create with no tensors -> (return code, message)"""
    c = fa.make_encoder_config(dict(CFG, **(cfg or {})))
    for k, v in over.items():
        setattr(c, k, v)
    h = C.c_void_p()
    rc = fa.lib().fl_encoder_create(C.byref(c), None, 0, dtype, 0, C.byref(h))
    assert rc != 0 and not h.value
    return rc, fa.lib().fl_last_error().decode()


def test_symbols_are_exported(fa):
    L = fa.lib()
    assert not [n for n in NEW if not hasattr(L, n)]
    out = subprocess.check_output(["nm", "-D", "--defined-only", fa.binding.LIB_PATH], text=True)
    for n in NEW:
        assert " T %s\n" % n in out, n
    assert fa.abi_version() == 2


def test_struct_layout_matches_the_header(fa, tmp_path):
    """sizeof / offsetof of fl_encoder_config as the C compiler sees the header against the ctypes mirror"""
    import os
    hdr = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "fastllm_mi355x.h")
    S = fa.FlEncoderConfig
    lines = ["#include <stddef.h>", '#include "%s"' % hdr,
             '_Static_assert(sizeof(fl_encoder_config) == %d, "sizeof");' % C.sizeof(S)]
    for name, _ in S._fields_:
        lines.append('_Static_assert(offsetof(fl_encoder_config, %s) == %d, "%s");' % (name, getattr(S, name).offset, name))
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines) + "\nint main(void) { return 0; }\n")
    r = subprocess.run(["gcc", "-std=c11", "-fsyntax-only", str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert C.sizeof(S) == 16 + 7 * 8 + 8 + 16
    assert (fa.binding.ACTIVATION["gelu_tanh"], fa.binding.ACTIVATION["gelu_erf"]) == (0, 1)


def test_config_errors_precede_the_device_probe(fa):
    # FL_ERR_BAD_CONFIG: heads do not divide hidden_size; a size that is not positive
    rc, msg = create(fa, dict(num_attention_heads=3))
    assert rc == -1 and "divisible" in msg
    for field in ("hidden_size", "intermediate_size", "num_hidden_layers", "num_attention_heads", "max_position_embeddings", "vocab_size"):
        for bad in (0, -4):
            assert create(fa, {field: bad})[0] == -1, (field, bad)
    assert create(fa, max_batch_tokens=-1)[0] == -1
    # FL_ERR_UNSUPPORTED: head_dim other than 32 / 64.  A hidden_size that is not a multiple of 8 cannot have such a head_dim, so it is
    # refused by the same check (132 / 4 = 33, 100 / 2 = 50); an intermediate_size that is not a multiple of 8 has a check of its own
    for bad in (dict(num_attention_heads=8), dict(num_attention_heads=1), dict(hidden_size=96, num_attention_heads=2),
                dict(hidden_size=132, num_attention_heads=4), dict(hidden_size=100, num_attention_heads=2)):
        rc, msg = create(fa, bad)
        assert rc == -10 and "head_dim" in msg, (bad, msg)
    for inter in (100, 511, 4):
        rc, msg = create(fa, dict(intermediate_size=inter))
        assert rc == -10 and "intermediate_size" in msg, (inter, msg)
    # FL_ERR_BAD_ARGUMENT: unknown activation, wrong struct_size, a compute dtype other than F32 / BF16
    rc, msg = create(fa, activation=2)
    assert rc == -8 and "activation" in msg
    assert create(fa, activation=-1)[0] == -8
    rc, msg = create(fa, struct_size=C.sizeof(fa.FlEncoderConfig) - 8)
    assert rc == -8 and "struct_size" in msg
    assert create(fa, struct_size=0)[0] == -8
    c = fa.make_encoder_config(CFG)                                     # _pad and _reserved must be 0
    for field, value in (("_pad", 1), ("_reserved", (C.c_int64 * 2)(0, 7)), ("_reserved", (C.c_int64 * 2)(-1, 0))):
        rc, msg = create(fa, **{field: value})
        assert rc == -8 and "_reserved" in msg, (field, msg)
    assert create(fa, dtype=2)[0] == -8                                 # FL_DTYPE_F16
    assert create(fa, dtype=7)[0] == -8


def test_null_pointers_are_rejected(fa):
    L = fa.lib()
    c = fa.make_encoder_config(CFG)
    assert L.fl_encoder_create(C.byref(c), None, 0, 1, 0, None) == -8       # FL_ERR_BAD_ARGUMENT, not a segfault
    assert b"null out" in L.fl_last_error()
    h = C.c_void_p()
    assert L.fl_encoder_create(None, None, 0, 1, 0, C.byref(h)) == -8
    ids = np.zeros(4, np.uint32)
    offs = np.array([0, 4], np.uint64)
    assert L.fl_encoder_hidden(None, ids.ctypes.data, 4, None) == -8
    assert b"null out" in L.fl_last_error()
    assert L.fl_encoder_embed(None, ids.ctypes.data, offs.ctypes.data, 1, None) == -8
    out = np.zeros(4, np.float32)
    assert L.fl_encoder_hidden(None, ids.ctypes.data, 4, out.ctypes.data) == -8          # null encoder
    assert L.fl_encoder_embed(None, ids.ctypes.data, offs.ctypes.data, 1, out.ctypes.data) == -8
    assert L.fl_op_encoder_attention(None, None, None, offs.ctypes.data, 1, 1, 32, 1, None) == -8
    L.fl_encoder_release(None)                                                           # a no-op


def test_op_attention_shape_errors_precede_the_device_probe(fa):
    q = np.zeros((4, 48), np.float32)
    with pytest.raises(fa.FastLLMError) as e:
        fa.op_encoder_attention(q, q, q, [4], 1, 48)
    assert e.value.code == -10
    q = np.zeros((4, 32), np.float32)
    with pytest.raises(fa.FastLLMError) as e:
        fa.op_encoder_attention(q, q, q, [4, 0], 1, 32)                                   # an empty sequence
    assert e.value.code == -8


def test_no_cpu_path(fa):
    """Without a GPU the encoder fails loudly; it never computes on the host."""
    if fa.device_count() > 0:
        pytest.skip("a GPU is visible here")
    w = bert_ref.synth_weights(CFG)
    with pytest.raises(fa.FastLLMError) as e:
        fa.Encoder(CFG, w)
    assert e.value.code == -9 and "no CPU path" in str(e.value)                           # FL_ERR_NO_DEVICE
    q = np.zeros((4, 32), np.float32)
    with pytest.raises(fa.FastLLMError) as e:
        fa.op_encoder_attention(q, q, q, [4], 1, 32)
    assert e.value.code == -9 and "no CPU path" in str(e.value)
