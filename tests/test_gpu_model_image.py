"""The model build on the device, bit for bit: convert_slice_kernel alone (fl_op_convert_slice) and every device tensor of built models
(fl_op_model_tensor) against the numpy restatement of tests/model_image_ref.py -- which tests/test_model_image_ref.py checks against
torch and against the source tensors.  Everything is compared exactly; a NaN may be any NaN; only the RoPE tables, which come from
the host's powf / cosf / sinf, have a (derived) tolerance.

Every model here is built with FL_DEBUG_POISON=255, so an element of a weight that no launch and no memset wrote is a NaN pattern
rather than whatever (often zero) the allocator handed back."""
import numpy as np
import pytest

import model_image_ref as ref
import synth
from test_model_image_ref import cfg_variant, f16_set, f32_set

pytestmark = pytest.mark.gpu
BAD, UNSUPPORTED = -8, -10


class Shared:
    """what the tests of this file share: the library, the full pattern sets and lazily made, cached synthetic weights"""

    def __init__(self, fa):
        self.fa = fa
        self.sets = {"f32": f32_set(), "f16": f16_set(), "bf16": f16_set()}
        self._w = {}

    def weights(self, cfg):
        key = tuple(sorted((k, v) for k, v in cfg.items()))
        if key not in self._w:
            self._w[key] = synth.synth_weights(cfg)
        return self._w[key]


@pytest.fixture(scope="module")
def sh():
    import fastllm_amd
    assert fastllm_amd.device_count() >= 1, "no MI355X visible"
    return Shared(fastllm_amd)


def as_src(bits, src_dtype):
    """pattern array -> what the binding takes for that source type"""
    return bits.view(np.float32) if src_dtype == "f32" else bits.view(np.float16) if src_dtype == "f16" else bits


# ---- the conversion kernel alone -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("src_dtype,dst_dtype", [("f32", "bf16"), ("f16", "bf16"), ("f16", "f32"), ("f32", "f32"), ("bf16", "bf16"), ("bf16", "f32")])
def test_conversion_on_the_full_sets(sh, src_dtype, dst_dtype):
    """f32 -> bf16 on the 5 x 65 536 patterns around every bf16 value (ties, subnormals, inf, NaN), f16 -> both on all 65 536 patterns,
    and the pairs that must not change a value on the same data"""
    u = sh.sets[src_dtype]
    R, Cc = u.shape
    got = sh.fa.op_convert_slice(as_src(u, src_dtype), 0, 0, R, Cc, dst_dtype, R, Cc)
    want = ref.convert(u, src_dtype, dst_dtype)
    assert ref.diff(got, want) == []
    assert np.array_equal(ref.is_nan(got), ref.is_nan(want))                # a NaN only where a NaN went in
    if dst_dtype == "f32":
        # ... and the fp32 copy of the ROUNDED value: how a bf16 model holds its norm weights and q/k/v biases
        got = sh.fa.op_convert_slice(as_src(u, src_dtype), 0, 0, R, Cc, "f32", R, Cc, via_bf16=True)
        want = ref.convert(ref.convert(u, src_dtype, "bf16"), "bf16", "f32")
        assert ref.diff(got, want) == [] and np.array_equal(ref.is_nan(got), ref.is_nan(want))
        assert not (got & 0xFFFF)[~ref.is_nan(got)].any()


# ---- the element map alone -------------------------------------------------------------------------------------------------------
def ids(rows, cols):
    """fp32 values that name their place: 1, 2, 3, ... (exact in fp32; as bf16 they round, which the restatement does too)"""
    return (np.arange(rows * cols, dtype=np.float32) + 1).reshape(rows, cols)


MAP_CASES = {
    # name: (source shape, (r0, c0, rows, cols), (dst_rows, dst_ld), dst_row0, row_mode, head_pad, dm, d)
    "slice_390_elements": ((40, 24), (3, 8, 30, 13), (40, 20), 5, 0, 0, 0, 0),           # dst_ld > cols, dst_row0 > 0, 390 % 256 != 0
    "slice_last_row_last_col": ((40, 24), (3, 8, 37, 16), (40, 17), 3, 0, 0, 0, 0),
    "one_element": ((40, 24), (39, 23, 1, 1), (3, 3), 1, 0, 0, 0, 0),
}
for _n in (40, 16, 17, 352):
    for _mode in (1, 2):
        MAP_CASES["%s_%d_rows" % ("gate" if _mode == 1 else "up", _n)] = ((_n, 24), (0, 0, _n, 24), ((_n + 15) // 16 * 32, 24), 0, _mode, 0, 0, 0)
MAP_CASES["gate_of_a_slice"] = ((40, 24), (3, 8, 37, 16), (96, 20), 0, 1, 0, 0, 0)
for _dm, _d in ((48, 64), (2, 64), (96, 128), (100, 128)):
    MAP_CASES["head_rows_%d_in_%d" % (_dm, _d)] = ((3 * _dm + 1, 24), (1, 8, 3 * _dm, 13), (3 * _d + 2, 15), 2, 0, 1, _dm, _d)
    MAP_CASES["head_cols_%d_in_%d" % (_dm, _d)] = ((11, 3 * _dm + 2), (1, 2, 10, 3 * _dm), (12, 3 * _d + 5), 1, 0, 2, _dm, _d)


@pytest.mark.parametrize("case", sorted(MAP_CASES))
def test_element_map(sh, case):
    """slice offsets, the destination's pitch and row offset, the gate/up interleave, padded heads in rows and in columns -- and
    every destination element outside the map still holds the 0xff pattern"""
    shape, (r0, c0, rows, cols), (dst_rows, dst_ld), dst_row0, row_mode, head_pad, dm, d = MAP_CASES[case]
    src = ids(*shape)
    for src_dtype, dst_dtype, via in (("f32", "f32", False), ("f32", "bf16", False), ("f16", "f32", False), ("bf16", "bf16", False), ("f32", "f32", True)):
        s = src if src_dtype == "f32" else (src % 2048).astype(np.float16) if src_dtype == "f16" else synth.f32_to_bf16_bits(src)
        got = sh.fa.op_convert_slice(s, r0, c0, rows, cols, dst_dtype, dst_rows, dst_ld, dst_row0, row_mode, head_pad, dm, d, via)
        want = ref.convert_slice(s, src_dtype, r0, c0, rows, cols, dst_dtype, dst_rows, dst_ld, dst_row0, row_mode, head_pad, dm, d, via)
        ones = 0xFFFFFFFF if dst_dtype == "f32" else 0xFFFF
        assert int((want != ones).sum()) == rows * cols and int((want == ones).sum()) == dst_rows * dst_ld - rows * cols
        assert np.array_equal(got, want), (case, src_dtype, dst_dtype, ref.diff(got, want))          # bits, the untouched all-ones included


def test_the_hook_refuses_what_would_leave_the_destination(sh):
    fa = sh.fa
    src = ids(40, 24)

    def refused(*a, **k):
        with pytest.raises(fa.FastLLMError) as e:
            fa.op_convert_slice(src, *a, **k)
        return e.value.code == BAD
    assert refused(3, 8, 38, 16, "bf16", 64, 64) and refused(3, 8, 37, 17, "bf16", 64, 64)            # the slice leaves the source
    assert refused(0, 0, 40, 24, "bf16", 39, 24) and refused(0, 0, 40, 24, "bf16", 40, 23) and refused(0, 0, 40, 24, "f32", 41, 24, 2)
    assert refused(0, 0, 40, 24, "bf16", 87, 24, 0, 2) and refused(0, 0, 40, 24, "bf16", 71, 24, 0, 1)  # row 39 is gate row 64 + 7, up row 87
    assert refused(0, 0, 40, 24, "bf16", 96, 24, 1, 1)                                                  # the interleave takes no row offset
    # 36 rows are 3 heads of 12 in 16: the last element at 32 + 8 + 5; 24 columns are 2 heads: 16 + 13
    assert refused(0, 0, 36, 24, "bf16", 45, 24, 0, 0, 1, 12, 16) and refused(0, 0, 40, 24, "bf16", 40, 29, 0, 0, 2, 12, 16)
    assert refused(0, 0, 40, 24, "bf16", 64, 64, 0, 0, 1, 12, 8) and refused(0, 0, 40, 24, "bf16", 64, 64, 0, 0, 2, 5, 8)
    got = fa.op_convert_slice(src, 0, 0, 40, 24, "f32", 40, 24)                                        # ... and the tight fit runs
    assert np.array_equal(got.view(np.float32), src)


# ---- model images ----------------------------------------------------------------------------------------------------------------
def tied(cfg, w):
    return {k: v for k, v in w.items() if k != "lm_head.weight"}


IMAGE_CASES = {
    # name: (config, drop lm_head.weight, tensor-parallel degrees)
    "llama_a": (synth.CONFIGS["llama_a"], False, (1, 2)),
    "qwen2_a": (synth.CONFIGS["qwen2_a"], False, (1, 2)),
    "qwen2_a_tied": (synth.CONFIGS["qwen2_a"], True, (1, 2)),
    "qwen2_a_tied_odd_vocab": (cfg_variant("qwen2_a", vocab_size=301), True, (1, 2)),
    "llama_d100": (synth.CONFIGS["llama_d100"], False, (1, 2)),
    "mistral_d48": (synth.CONFIGS["mistral_d48"], False, (1, 2)),
    "qwen2_d96": (synth.CONFIGS["qwen2_d96"], False, (1, 2)),
    "llama_tp4": (synth.CONFIGS["llama_tp4"], False, (4,)),
    "llama_a_i360": (cfg_variant("llama_a", intermediate_size=360), False, (1, 2)),
}
# (source type, compute dtype, the tensor whose first row carries the special values -- for models with q/k/v bias, a bias)
BUILDS = {
    "f32_to_bf16": ("f32", "bf16", "model.layers.0.self_attn.q_proj.weight", "model.layers.1.self_attn.q_proj.bias"),
    "f16_to_bf16": ("f16", "bf16", "model.layers.1.post_attention_layernorm.weight", "model.layers.0.self_attn.v_proj.bias"),
    "bf16_to_bf16": ("bf16", "bf16", "model.embed_tokens.weight", "model.layers.1.mlp.down_proj.weight"),
    "f16_to_f32": ("f16", "f32", "model.layers.1.mlp.down_proj.weight", "model.norm.weight"),
}
NORMS = ("model.norm.weight", "model.layers.1.post_attention_layernorm.weight")


def build(fa, cfg, w, dtype, tp, **kw):
    if tp == 1:
        return fa.Model(cfg, w, dtype=dtype, **kw)
    return fa.Model(cfg, w, dtype=dtype, tp_mode=fa.binding.TP_EMULATED, tp_size=tp, **kw)


def check_image(m, want, shard, what):
    """every selector of `want` (the restatement's dict) against the device tensor of local shard `shard`"""
    for key, w in want.items():
        name, layer = (key, 0) if isinstance(key, str) else key
        r, c, _ = m.tensor(name, layer, shard, shape_only=True)
        assert (r, c) == w.shape, (what, key, (r, c), w.shape)
        got = m.tensor(name, layer, shard)
        assert ref.diff(got, w) == [], (what, "shard %d" % shard, key, ref.diff(got, w))


@pytest.mark.parametrize("build_name", sorted(BUILDS))
@pytest.mark.parametrize("case", sorted(IMAGE_CASES))
def test_model_image(sh, monkeypatch, case, build_name):
    """every device tensor of every shard: the conversion of the source (rounded where it must be), the fused q | k | v rows, the padded
    heads, the gate/up interleave with its padding, the tensor-parallel slices, the tied lm_head, biases and norms in fp32"""
    fa = sh.fa
    cfg, drop_lm_head, tps = IMAGE_CASES[case]
    src_dtype, dtype, special, special_bias = BUILDS[build_name]
    has_bias = ref.dims(cfg)["bias"]
    w = ref.rounding_sources(sh.weights(cfg), src_dtype, special_bias if has_bias else special, finite_only=NORMS)
    if drop_lm_head:
        w = tied(cfg, w)
    monkeypatch.setenv("FL_DEBUG_POISON", "255")
    for tp in tps:
        m = build(fa, cfg, w, dtype, tp)
        try:
            for rank in range(tp):
                want = ref.model_image(cfg, w, dtype, tp, rank)
                assert len(want) == 3 + ref.dims(cfg)["L"] * (7 if has_bias else 6)
                check_image(m, want, rank, (case, build_name, "tp %d" % tp))
            # what this model does not have, and the hook's own argument errors
            for bad in (dict(name="wqkv_q"), dict(name="lm_head_s"), dict(name="wqkv", layer=cfg["num_hidden_layers"]), dict(name="ln2", layer=-1),
                        dict(name="embed", shard=tp), dict(name="embed", shard=-1), dict(name=22), dict(name=-1)) + (() if has_bias else (dict(name="bqkv"),)):
                with pytest.raises(fa.FastLLMError) as e:
                    m.tensor(shape_only=True, **bad)
                assert e.value.code == BAD, bad
            assert m.tensor("embed", layer=99, shape_only=True) == (cfg["vocab_size"], cfg["hidden_size"], 1 if dtype == "bf16" else 0)   # (layer: per-layer selectors only)
        finally:
            m.close()


@pytest.mark.parametrize("case", ["llama_a", "mistral_a", "llama_d100_i360"])
def test_model_image_e4m3(sh, monkeypatch, case):
    """FL_WEIGHTS_E4M3_ROW: every projection quantised in its FINAL layout -- the row scales sit at the interleaved / padded rows, a zero
    padding row has scale 1 and zero bytes -- and the bf16 weights replaced by s * q"""
    fa = sh.fa
    cfg = cfg_variant("llama_d100", intermediate_size=360) if case == "llama_d100_i360" else synth.CONFIGS[case]
    w = sh.weights(cfg)
    monkeypatch.setenv("FL_DEBUG_POISON", "255")
    m = fa.Model(cfg, w, dtype="bf16", decode_weights="e4m3")
    try:
        want = ref.model_image(cfg, w, "bf16", 1, 0, e4m3=True)
        assert len(want) == 3 + 2 + cfg["num_hidden_layers"] * (6 + 8)
        check_image(m, want, 0, (case, "e4m3"))
        assert m.tensor("wgu_q", shape_only=True)[2] == fa.ELEM_E4M3 and m.tensor("wgu_s", 1).dtype == np.float32
    finally:
        m.close()


@pytest.mark.parametrize("case", ["llama_a", "mistral_a"])
def test_model_image_e4m3_tp2_is_refused(sh, case):
    """The library does not build FP8 images under tensor parallelism (fl_model_create_opts refuses the pair before it touches the
    device; tests/test_w8_abi.py pins the refusal), so at tp 2 there is no image to compare: the restatement's tp 2 image is checked on
    the CPU (tests/test_model_image_ref.py) and the device side must keep refusing rather than build something unchecked."""
    fa = sh.fa
    cfg = synth.CONFIGS[case]
    with pytest.raises(fa.FastLLMError) as e:
        build(fa, cfg, sh.weights(cfg), "bf16", 2, decode_weights="e4m3")
    assert e.value.code == UNSUPPORTED and "tensor parallelism" in str(e.value)
    want = [ref.model_image(cfg, sh.weights(cfg), "bf16", 2, r, e4m3=True) for r in range(2)]
    assert ref.diff(want[0]["wgu_s", 0], want[1]["wgu_s", 0])                                          # (each rank's rows have scales of their own)


# ---- RoPE tables -----------------------------------------------------------------------------------------------------------------
ROPE_CASES = {"llama_a": synth.CONFIGS["llama_a"], "llama_d100": synth.CONFIGS["llama_d100"],
              "qwen2_a_32k_theta_1e6": cfg_variant("qwen2_a", max_position_embeddings=32768)}


@pytest.mark.parametrize("case", sorted(ROPE_CASES))
def test_rope_tables(sh, monkeypatch, case):
    """cos / sin [max_pos][d/2] against fp64 cos / sin of the fp32 angle the restatement computes.  Exact: position 0 and every padded
    pair.  Bounded elsewhere by 2^-23 + |angle| * 2^-22 (2^-23 in column 0) -- derived in model_image_ref.rope_tables, not measured."""
    fa = sh.fa
    cfg = ROPE_CASES[case]
    D = ref.dims(cfg)
    assert D["max_pos"] == (32768 if "32k" in case else 512) and D["theta"] == (1e6 if "qwen2" in case else 1e4)
    cos, sin, bound, ang = ref.rope_tables(cfg)
    monkeypatch.setenv("FL_DEBUG_POISON", "255")
    tp = 2 if case == "llama_a" else 1
    m = build(fa, cfg, sh.weights(cfg), "bf16", tp)
    try:
        half, half_m = D["d"] // 2, D["dm"] // 2
        for shard in range(tp):
            for name, want in (("cos_tab", cos), ("sin_tab", sin)):
                got = m.tensor(name, shard=shard)
                assert got.shape == (D["max_pos"], half) and got.dtype == np.float32
                exact_one = 1.0 if name == "cos_tab" else 0.0
                assert (got[0] == exact_one).all() and (got[:, half_m:] == exact_one).all()
                err = np.abs(got.astype(np.float64) - want)
                ratio = np.divide(err, bound, out=np.zeros_like(err), where=bound > 0)
                worst = np.unravel_index(np.argmax(ratio), ratio.shape)
                print("%s %s shard %d: worst err / bound %.3f at position %d, pair %d (angle %.6g, err %.3g); column 0 worst %.3f"
                      % (case, name, shard, ratio[worst], worst[0], worst[1], ang[worst], err[worst], ratio[:, 0].max()))
                assert (err <= bound).all(), (name, worst, float(err[worst]), float(bound[worst]))
    finally:
        m.close()
