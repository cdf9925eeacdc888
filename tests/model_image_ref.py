"""A numpy restatement of the model build (fastllm_amd/csrc/weights.hip and convert_slice_kernel in k_ops.hip), written from the layout
description at the top of weights.hip: what every device tensor of a built model must hold, bit for bit.  It calls nothing of the
library (not fl_tp_slice either), so it is an independent witness; tests/test_model_image_ref.py checks it against torch and against
itself, tests/test_gpu_model_image.py compares the device with it.

Arrays of weights are BIT PATTERNS throughout: uint32 for fp32, uint16 for bf16 and f16.  Sources may also be given as float32 /
float16 arrays (viewed, not converted); a uint16 source is bf16 unless src_dtype says "f16".
"""
import numpy as np

ES = {"f32": np.uint32, "bf16": np.uint16, "f16": np.uint16}


def src_dtype_of(a):
    a = np.asarray(a)
    return {np.dtype(np.float32): "f32", np.dtype(np.uint32): "f32", np.dtype(np.float16): "f16", np.dtype(np.uint16): "bf16"}[a.dtype]


def _bits(a, src_dtype):
    a = np.ascontiguousarray(a)
    if a.dtype == np.float32:
        assert src_dtype == "f32"
        return a.view(np.uint32)
    if a.dtype == np.float16:
        assert src_dtype == "f16"
        return a.view(np.uint16)
    assert a.dtype == ES[src_dtype], (a.dtype, src_dtype)
    return a


def f32_bits_to_bf16_bits(u):
    """round-to-nearest-even on the fp32 value; subnormals, +-0 and +-inf kept; NaN in, (quiet) NaN out"""
    u = np.ascontiguousarray(u, dtype=np.uint32)
    nan = (u & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000)
    r = (u.astype(np.uint64) + 0x7FFF + ((u >> 16) & 1)) >> 16          # (64 bits: the increment may carry out of 0xffffxxxx, a NaN anyway)
    return np.where(nan, (u >> 16) | 0x40, r).astype(np.uint16)


def convert(a, src_dtype, dst_dtype):
    """Element-wise conversion of the build: src_dtype f32 / bf16 / f16 -> dst_dtype bf16 / f32.  Returns bit patterns (uint16 / uint32).
    Every source value is first the fp32 value it denotes (bf16 and f16 -> f32 are exact), then rounded once if the target is bf16."""
    u = _bits(a, src_dtype)
    if src_dtype == "bf16":
        f = u.astype(np.uint32) << 16
    elif src_dtype == "f16":
        f = u.view(np.float16).astype(np.float32).view(np.uint32)          # exact, subnormals included
    else:
        f = u
    assert dst_dtype in ("bf16", "f32")
    return f32_bits_to_bf16_bits(f) if dst_dtype == "bf16" else np.ascontiguousarray(f, dtype=np.uint32)


def is_nan(bits):
    """NaN-ness of a pattern array by its width: 2 bytes bf16, 4 bytes fp32 (float32 arrays are viewed), 1 byte: never"""
    b = np.asarray(bits)
    if b.dtype == np.float32:
        b = b.view(np.uint32)
    if b.dtype == np.uint16:
        return (b & 0x7FFF) > 0x7F80
    if b.dtype == np.uint32:
        return (b & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000)
    return np.zeros(b.shape, bool)


def diff(got, want, limit=5):
    """[] when `got` is `want`: same shape, same width, NaN where `want` has NaN (payload and sign of a NaN are not compared), the same
    bits everywhere else.  Otherwise a list of messages naming the count and the first few places."""
    got, want = np.asarray(got), np.asarray(want)
    if got.dtype == np.float32:
        got = got.view(np.uint32)
    if want.dtype == np.float32:
        want = want.view(np.uint32)
    if got.shape != want.shape or got.dtype != want.dtype:
        return ["shape / element type: got %s %s, want %s %s" % (got.shape, got.dtype, want.shape, want.dtype)]
    wn, gn = is_nan(want), is_nan(got)
    bad = np.where(wn, ~gn, got != want)
    if not bad.any():
        return []
    idx = np.argwhere(bad)
    out = ["%d of %d elements differ" % (len(idx), want.size)]
    for i in idx[:limit]:
        i = tuple(int(x) for x in i)
        out.append("  at %s: got 0x%x, want 0x%x" % (i, int(got[i]), int(want[i])))
    return out


# ---- sources that make the build's conversion round ----------------------------------------------------------------------------
def f32_special_values(n):
    """n fp32 patterns (n >= 64) spread over the full set of tests/test_model_image_ref.py: around bf16 values b drawn from every class
    -- zeros, subnormals, the smallest and largest normals, ordinary values, inf, NaN, both signs -- the patterns (b << 16) + {0, 0x7fff,
    0x8000, 0x8001, 0xffff}"""
    cls = [0x0000, 0x0001, 0x007F, 0x0080, 0x0081, 0x3F7F, 0x3F80, 0x3F81, 0x4049, 0x7F7E, 0x7F7F, 0x7F80, 0x7F81, 0x7FC0, 0x7FFF]
    b = np.array(cls + [x | 0x8000 for x in cls], dtype=np.uint32)
    pats = np.concatenate([(b << 16) + o for o in (0, 0x7FFF, 0x8000, 0x8001, 0xFFFF)]).astype(np.uint32)
    assert n >= 64
    return np.resize(pats, n)


def f16_special_values(n):
    """n f16 patterns: zeros, the smallest / a middle / the largest subnormal, the smallest normal, values whose fp32 image is a bf16
    tie or next to one, the largest finite value, inf, NaN; both signs"""
    cls = [0x0000, 0x0001, 0x0008, 0x0200, 0x03FF, 0x0400, 0x0401, 0x3C00, 0x3C03, 0x3C04, 0x3C05, 0x3C0C, 0x4248, 0x7BFF, 0x7C00, 0x7C01, 0x7E00,
           0x7FFF]
    pats = np.array(cls + [x | 0x8000 for x in cls], dtype=np.uint16)
    return np.resize(pats, n)


def rounding_sources(weights_bf16, src_dtype, special, finite_only=(), special_row=True):
    """Source tensors that the build has to ROUND, out of bf16-valued ones (dict name -> uint16 bits, tests/synth.py):
      "f32"   every value times 1 + 2^-10: no longer a bf16 value (it lies 1/8 .. 1/4 ulp above one in magnitude, so it rounds toward
              zero); the tensor `special` and every norm weight and bias times 1 + 3 * 2^-9 instead (3/8 .. 3/4 ulp: about half of
              them round away from zero, so rounding shows against truncation);
      "f16"   every value rounded to f16, then 0 .. 7 added to the pattern (f16 keeps three more significand bits than bf16: all eight
              residues, the tie among them) where that stays finite;
      "bf16"  the values as they are.
    The first row of `special` (a norm weight: its first elements) carries the special values above -- without NaN and inf for a
    tensor named in finite_only (norm weights), and not at all with special_row=False (models whose logits are compared)."""
    out = {}
    for name, bits in weights_bf16.items():
        f = (np.asarray(bits).astype(np.uint32) << 16).view(np.float32)
        if src_dtype == "f32":
            a = (f * np.float32(1 + 3 * 2.0 ** -9 if name == special or f.ndim == 1 else 1 + 2.0 ** -10)).astype(np.float32)
        elif src_dtype == "f16":
            u = f.astype(np.float16).view(np.uint16)
            bump = (np.arange(u.size, dtype=np.uint32).reshape(u.shape) % 8).astype(np.uint16)
            u = np.where((u & 0x7FFF) + bump < 0x7C00, u + bump, u).astype(np.uint16)
            a = u.view(np.float16)
        else:
            a = np.asarray(bits, dtype=np.uint16).copy()
        if name == special and special_row:
            a = a.copy()
            row = a.reshape(-1) if a.ndim == 1 else a[0]
            if src_dtype == "f32":
                sp = f32_special_values(row.size)
            elif src_dtype == "f16":
                sp = f16_special_values(row.size)
            else:
                sp = f32_bits_to_bf16_bits(f32_special_values(row.size) & np.uint32(0xFFFF0000))
            if name in finite_only:
                lim = 0x7F800000 if src_dtype == "f32" else 0x7C00 if src_dtype == "f16" else 0x7F80
                mask = 0x7FFFFFFF if src_dtype == "f32" else 0x7FFF
                sp = np.where((sp & mask) >= lim, sp & ~np.asarray(mask ^ (mask >> 2), sp.dtype), sp).astype(sp.dtype)
            row[:] = sp.view(row.dtype) if row.dtype != sp.dtype else sp
        out[name] = a
    return out


# ---- the element map of convert_slice_kernel -------------------------------------------------------------------------------------
def gateup_row(r, up):
    return (r // 16) * 32 + r % 16 + 16 * up


def padded_index(x, dm, d):
    """element x of a run of heads of dm -> its place in a run of heads of d: j stays (first half) or goes to d/2 + j - dm/2"""
    hd, j = divmod(x, dm)
    return hd * d + (j if j < dm // 2 else d // 2 + j - dm // 2)


def convert_slice(src, src_dtype, r0, c0, rows, cols, dst_dtype, dst_rows, dst_ld, dst_row0=0, row_mode=0, head_pad=0, dm=0, d=0, via_bf16=False):
    """The whole destination [dst_rows, dst_ld] after one launch into a buffer of 0xff bytes.  via_bf16 (fp32 destinations): the value
    rounded to bf16 first."""
    s = _bits(src, src_dtype)[r0:r0 + rows, c0:c0 + cols]
    s = convert(convert(s, src_dtype, "bf16"), "bf16", "f32") if via_bf16 and dst_dtype == "f32" else convert(s, src_dtype, dst_dtype)
    out = np.full((dst_rows, dst_ld), 0xFFFFFFFF if dst_dtype == "f32" else 0xFFFF, ES[dst_dtype])
    if head_pad == 1:
        dr = [dst_row0 + padded_index(r, dm, d) for r in range(rows)]
    elif row_mode == 0:
        dr = [dst_row0 + r for r in range(rows)]
    else:
        dr = [gateup_row(r, row_mode - 1) for r in range(rows)]
    dc = [padded_index(c, dm, d) for c in range(cols)] if head_pad == 2 else list(range(cols))
    assert max(dr) < dst_rows and max(dc) < dst_ld
    out[np.ix_(dr, dc)] = s
    return out


# ---- the device image of a model ------------------------------------------------------------------------------------------------
def dims(cfg, tp=1, rank=0):
    h, inter, V, L, H = (cfg[k] for k in ("hidden_size", "intermediate_size", "vocab_size", "num_hidden_layers", "num_attention_heads"))
    Hkv = cfg.get("num_key_value_heads") or H
    dm = h // H
    D = dict(h=h, inter=inter, V=V, L=L, H=H, Hkv=Hkv, dm=dm, d=64 if dm <= 64 else 128, Hs=H // tp, Hkvs=Hkv // tp, Is=inter // tp)
    assert H % tp == 0 and Hkv % tp == 0 and inter % tp == 0 and dm % 2 == 0 and dm <= 128
    D["Ip"] = (D["Is"] + 15) // 16 * 16
    vp = tp > 1 and V % tp == 0
    D["Vs"], D["v0"] = (V // tp, V // tp * rank) if vp else (V, 0)
    D["bias"] = bool(cfg.get("qkv_bias", cfg["family"] == "qwen2"))
    D["max_pos"], D["theta"] = cfg["max_position_embeddings"], cfg.get("rope_theta") or 10000.0
    return D


def _pad_heads(a, dm, d, axis):
    """heads of dm along `axis` -> heads of d: [first half | zeros | second half | zeros]"""
    n = a.shape[axis] // dm
    idx = [padded_index(x, dm, d) for x in range(n * dm)]
    shape = list(a.shape)
    shape[axis] = n * d
    out = np.zeros(shape, a.dtype)
    if axis == 0:
        out[idx] = a
    else:
        out[:, idx] = a
    return out


SCALED = ("wqkv", "wo", "wgu", "wd", "lm_head")                  # the projections an FL_WEIGHTS_E4M3_ROW model quantises


def model_image(cfg, weights, compute_dtype, tp=1, rank=0, e4m3=False):
    """dict selector -> expected array of tensor-parallel rank `rank` of `tp`: "embed", "norm", "lm_head", and per layer (name, l) for
    "wqkv", "bqkv" (with q/k/v bias), "wo", "wgu", "wd", "ln1", "ln2".  Weights are bit patterns of compute_dtype ("bf16" / "f32");
    norms and biases fp32 patterns [n, 1] of the value in compute_dtype -- the reference casts EVERY tensor of the checkpoint to the
    model's dtype (VarBuilder::from_tensors(tensors, dtype, device)), so a bf16 model's norm weights are bf16 values.  Megatron partition: q / k / v / gate / up / lm_head by rows, o / down by columns; the
    embedding and the norms whole.  With e4m3: every projection, in its final layout, also as (name + "_q"[, l]) e4m3 bytes and
    (name + "_s"[, l]) fp32 row scales [rows, 1], and the bf16 image itself becomes s * q."""
    D = dims(cfg, tp, rank)
    dm, d, Hs, Hkvs, Is, Ip, h = D["dm"], D["d"], D["Hs"], D["Hkvs"], D["Is"], D["Ip"], D["h"]

    def cv(name, dst=compute_dtype):
        a = np.asarray(weights[name])
        b = convert(a, src_dtype_of(a), compute_dtype)
        if dst != compute_dtype:                        # norms and biases: the model's (rounded) value, held in fp32
            b = convert(b, compute_dtype, dst)
        return b.reshape(-1, 1) if b.ndim == 1 else b

    img = {"embed": cv("model.embed_tokens.weight"), "norm": cv("model.norm.weight", "f32")}
    if "lm_head.weight" in weights:
        lm = cv("lm_head.weight")
    else:
        assert cfg["family"] == "qwen2", "only Qwen2 checkpoints may lack lm_head.weight"
        lm = img["embed"]
    img["lm_head"] = lm[D["v0"]:D["v0"] + D["Vs"]].copy()
    for l in range(D["L"]):
        p = "model.layers.%d." % l

        def qkv(kind, dst=compute_dtype):
            parts = []
            for nm, n in (("q_proj", Hs), ("k_proj", Hkvs), ("v_proj", Hkvs)):
                a = cv(p + "self_attn." + nm + kind, dst)
                parts.append(_pad_heads(a[rank * n * dm:(rank + 1) * n * dm], dm, d, 0))
            return np.concatenate(parts, axis=0)
        img["wqkv", l] = qkv(".weight")
        if D["bias"]:
            img["bqkv", l] = qkv(".bias", "f32")
        img["wo", l] = _pad_heads(cv(p + "self_attn.o_proj.weight")[:, rank * Hs * dm:(rank + 1) * Hs * dm], dm, d, 1)
        gate, up = cv(p + "mlp.gate_proj.weight"), cv(p + "mlp.up_proj.weight")
        wgu = np.zeros((2 * Ip, h), gate.dtype)
        for r in range(Is):
            wgu[gateup_row(r, 0)] = gate[rank * Is + r]
            wgu[gateup_row(r, 1)] = up[rank * Is + r]
        img["wgu", l] = wgu
        wd = np.zeros((h, Ip), gate.dtype)
        wd[:, :Is] = cv(p + "mlp.down_proj.weight")[:, rank * Is:(rank + 1) * Is]
        img["wd", l] = wd
        img["ln1", l], img["ln2", l] = cv(p + "input_layernorm.weight", "f32"), cv(p + "post_attention_layernorm.weight", "f32")
    if e4m3:
        from test_w8_abi import dequantize, quantize_rows_ref
        assert compute_dtype == "bf16"
        for key in [k for k in img if (k if isinstance(k, str) else k[0]) in SCALED]:
            q, s = quantize_rows_ref(convert(img[key], "bf16", "f32").view(np.float32))
            back = convert(dequantize(q, s), "f32", "bf16")
            name, tail = (key, ()) if isinstance(key, str) else (key[0], key[1:])
            img[key] = back
            img[(name + "_q",) + tail if tail else name + "_q"] = q
            img[(name + "_s",) + tail if tail else name + "_s"] = s.reshape(-1, 1).astype(np.float32).view(np.uint32)
    return img


def rope_tables(cfg):
    """The fp32 chain of build_rope restated -- inv[j] = 1 / powf(theta, 2j / dm) for j < dm/2, angle = (float)p * inv[j] -- and what a
    table may hold: (cos, sin, bound, angle), float64 [max_pos, d/2].  cos / sin are taken in fp64 of the fp32 angle.  bound is the
    allowed |error| per element: 2^-23 + |angle| * 2^-22 (one ulp of cosf / sinf near 1, plus one ulp of powf disagreement in inv and
    the product's rounding, both carried through the angle: d cos / d angle <= 1); 2^-23 alone in column 0, where inv is exactly 1 and
    the angle exactly p; 0 -- exact cos 1, sin 0 -- in row 0 and in every padded pair j >= dm/2."""
    D = dims(cfg)
    half, half_m, P = D["d"] // 2, D["dm"] // 2, D["max_pos"]
    theta = np.float32(D["theta"])
    j = np.arange(half_m)
    inv = (np.float32(1.0) / np.power(theta, (2 * j).astype(np.float32) / np.float32(D["dm"]), dtype=np.float32)).astype(np.float32)
    ang32 = np.zeros((P, half), np.float32)
    ang32[:, :half_m] = np.arange(P, dtype=np.float32)[:, None] * inv[None, :]
    ang = ang32.astype(np.float64)
    bound = 2.0 ** -23 + np.abs(ang) * 2.0 ** -22
    bound[:, 0] = 2.0 ** -23
    bound[:, half_m:] = 0.0
    bound[0, :] = 0.0
    return np.cos(ang), np.sin(ang), bound, ang
