"""The FP8 weight mode (FL_WEIGHTS_E4M3_ROW) without a GPU: the three new entry points are exported and declared, fl_model_options has
the header's size, and every refusal that needs no device is decided before the device probe.  Also the yardstick of the GPU
tests: a torch / numpy restatement of the quantiser

    W'[n,k] = s[n] * q[n,k],   s[n] = 2^e, e the smallest integer with absmax(W[n,:]) / 2^e <= 448 (zero row: s = 1),
    q[n,k] = RNE_e4m3fn(W[n,k] / s[n])                      (the division is by a power of two: exact)

with its own checks (tests/test_gpu_w8_ops.py and tests/test_gpu_w8_parity.py import it)."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "fastllm_mi355x.h")
PROJECTIONS = ("q_proj.weight", "k_proj.weight", "v_proj.weight", "o_proj.weight", "gate_proj.weight", "up_proj.weight",
               "down_proj.weight", "lm_head.weight")


# ---- the restatement ---------------------------------------------------------------------------------------------------------
def quantize_rows_ref(w):
    """w float32 [N,K] -> (q uint8 [N,K] e4m3fn codes, s float32 [N])."""
    import torch
    w = np.ascontiguousarray(w, dtype=np.float32)
    amax = np.abs(w).max(axis=1)
    m, x = np.frexp(amax)                                  # amax = m * 2^x, m in [0.5, 1); 448 = 0.875 * 2^9
    e = np.where(m <= 0.875, x - 9, x - 8)
    e = np.where(amax == 0, 0, np.maximum(e, -126)).astype(np.int32)     # (exponent floor: s stays a normal fp32)
    s = np.ldexp(np.float32(1.0), e).astype(np.float32)
    scaled = torch.from_numpy(w / s[:, None])              # exact: a power of two
    q = scaled.to(torch.float8_e4m3fn).view(torch.uint8).numpy()
    return q, s


def e4m3_to_f32(q):
    import torch
    return torch.from_numpy(np.ascontiguousarray(q, dtype=np.uint8)).view(torch.float8_e4m3fn).to(torch.float32).numpy()


def dequantize(q, s):
    return e4m3_to_f32(q) * s[:, None]


def dequantized_weights(w):
    """synth weights (bf16 bits) -> the bf16 bits of W' for every projection matrix (embedding, norms and biases unchanged): the bf16
    model an FP8 model must equal."""
    out = {}
    for name, bits in w.items():
        if name.endswith(PROJECTIONS):
            q, s = quantize_rows_ref(synth.bf16_bits_to_f32(bits))
            wp = dequantize(q, s)
            back = synth.f32_to_bf16_bits(wp)
            assert np.array_equal(synth.bf16_bits_to_f32(back), wp), name       # s * q is exact in bf16
            out[name] = back
        else:
            out[name] = bits
    return out


def _sample_matrix():
    rs = np.random.RandomState(11)
    w = (rs.standard_normal((512, 4096)) * 0.02).astype(np.float32)
    w[7] = 0.0                                             # a zero row (head_dim padding)
    w[9, 100] = 3.0                                        # an outlier
    w[11] *= 448.0 * 2.0 ** -7 / np.abs(w[11]).max()       # absmax exactly 448 * 2^e
    return w


def test_restatement_scale_range_and_codes():
    w = _sample_matrix()
    q, s = quantize_rows_ref(w)
    amax = np.abs(w).max(axis=1)
    nz = amax > 0
    r = amax[nz] / s[nz]
    assert (r > 224).all() and (r <= 448).all(), (r.min(), r.max())
    assert s[7] == 1.0 and (q[7] == 0).all()
    assert np.array_equal(np.frexp(s)[0], np.full_like(s, 0.5))                 # powers of two
    assert not ((q & 0x7F) == 0x7F).any()                                       # no NaN code
    assert np.abs(w[11]).max() / s[11] == 448.0 and (q[11] & 0x7F).max() == 0x7E


def test_restatement_image_is_exact_in_bf16():
    w = _sample_matrix()
    q, s = quantize_rows_ref(w)
    wp = dequantize(q, s)
    assert np.array_equal(synth.bf16_bits_to_f32(synth.f32_to_bf16_bits(wp)), wp)
    rel = np.linalg.norm(wp - w) / np.linalg.norm(w)
    print("relative L2 of the format on N(0, 0.02^2): %.3e" % rel)             # a property of e4m3, not bounded here
    # quantising the image again changes nothing: W' is a fixed point (same scale, same codes)
    q2, s2 = quantize_rows_ref(wp)
    assert np.array_equal(q2, q) and np.array_equal(s2, s)


def test_restatement_rounds_ties_to_even_and_keeps_subnormals():
    # one row, absmax 448 -> s = 1; e4m3 neighbours around 17: 16, 18 (3 mantissa bits at 2^4: step 2); 17 is a tie -> 16 (even mantissa)
    row = np.zeros((1, 64), dtype=np.float32)
    row[0, :8] = [448.0, 17.0, 19.0, 2.0 ** -9, 2.0 ** -10, 3 * 2.0 ** -10, 2.0 ** -7 + 2.0 ** -10, -17.0]
    q, s = quantize_rows_ref(row)
    assert s[0] == 1.0
    got = e4m3_to_f32(q)[0, :8]
    assert list(got) == [448.0, 16.0, 20.0, 2.0 ** -9, 0.0, 2.0 ** -8, 2.0 ** -7, -16.0], got


# ---- the ABI surface ----------------------------------------------------------------------------------------------------------
class Options(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("decode_weights", C.c_int32), ("_reserved", C.c_int64 * 3)]


@pytest.fixture(scope="module")
def L():
    import fastllm_amd
    return fastllm_amd.lib()


def test_new_symbols_are_exported_and_declared(L):
    hdr = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name in ("fl_model_create_opts", "fl_op_quantize_rows", "fl_op_gemv_w8"):
        assert hasattr(L, name), name
        assert re.search(r"\b%s\s*\(" % name, hdr), name
    assert "FL_WEIGHTS_COMPUTE_DTYPE = 0" in hdr and "FL_WEIGHTS_E4M3_ROW = 1" in hdr
    assert L.fl_abi_version() == 2


def test_options_struct_size_matches_the_header():
    import fastllm_amd.binding as B
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "s.c"), os.path.join(d, "s")
        open(src, "w").write('#include <stdio.h>\n#include "%s"\nint main(void) { printf("%%zu %%zu\\n", sizeof(fl_model_options), sizeof(fl_model_info)); return 0; }\n' % HEADER)
        subprocess.run(["gcc", "-std=c11", src, "-o", exe], check=True)
        so, si = (int(x) for x in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split())
    assert so == C.sizeof(Options) == C.sizeof(B.FlModelOptions) == 32
    assert si == C.sizeof(B.FlModelInfo)
    assert B.FlModelInfo.decode_weights.offset == si - 4


def _create(L, dtype, decode_weights, struct_size=None, tp=None, opts=True):
    import fastllm_amd.binding as B
    cfg = B.make_config(synth.CONFIGS["llama_a"])
    o = Options(C.sizeof(Options) if struct_size is None else struct_size, decode_weights)
    par = B.FlParallel()
    if tp:
        par.mode, par.tp_size = B.TP_EMULATED, tp
    h = C.c_void_p()
    rc = L.fl_model_create_opts(C.byref(cfg), None, 0, dtype, C.byref(par) if tp else None, C.cast(C.byref(o), C.POINTER(B.FlModelOptions)) if opts else None,
                                C.byref(h))
    return rc, L.fl_last_error().decode()


def test_refusals_come_before_the_device_probe(L):
    """Valid config, no tensors: a good request ends in FL_ERR_NO_DEVICE (-9) on a machine without a GPU or FL_ERR_MISSING_TENSOR (-2) on
    one with; the refusals below must not get that far."""
    import fastllm_amd.binding as B
    rc, msg = _create(L, B.BF16, 7)
    assert rc == -8 and "decode_weights" in msg, (rc, msg)
    rc, msg = _create(L, B.BF16, 1, struct_size=24)
    assert rc == -8 and "struct_size" in msg, (rc, msg)
    rc, msg = _create(L, B.F32, 1)
    assert rc == -10 and "BF16" in msg, (rc, msg)
    rc, msg = _create(L, B.BF16, 1, tp=2)
    assert rc == -10 and "tensor parallelism" in msg, (rc, msg)
    cfg = B.make_config(dict(synth.CONFIGS["llama_a"], hidden_size=264, num_attention_heads=4, num_key_value_heads=2))      # a multiple of 8, not of 16
    o, h = Options(C.sizeof(Options), 1), C.c_void_p()
    rc = L.fl_model_create_opts(C.byref(cfg), None, 0, B.BF16, None, C.cast(C.byref(o), C.POINTER(B.FlModelOptions)), C.byref(h))
    assert rc == -10 and "multiple of 16" in L.fl_last_error().decode()
    # a good request, and NULL options (= fl_model_create), pass every one of those checks
    for rc, _ in (_create(L, B.BF16, 1), _create(L, B.BF16, 0), _create(L, B.BF16, 0, opts=False)):
        assert rc in (-9, -2), rc


def test_binding_passes_the_option_through():
    import fastllm_amd as fa
    cfg = synth.CONFIGS["llama_a"]
    with pytest.raises(fa.FastLLMError) as e:
        fa.Model(cfg, {}, dtype="f32", decode_weights="e4m3")
    assert e.value.code == -10
    with pytest.raises(fa.FastLLMError) as e:
        fa.Model(cfg, {}, dtype="bf16", decode_weights=5)
    assert e.value.code == -8
