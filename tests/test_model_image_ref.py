"""The restatement of the model build (tests/model_image_ref.py) checked without a GPU: its conversions against torch's CPU casts on
full sets of patterns, its images against the source tensors (every source element exactly once over the ranks, all padding zero),
and its diff() against the mistakes a build could make without moving whole-model logits past their tolerance."""
import numpy as np
import pytest

import model_image_ref as ref
import synth


def f32_set():
    """for every bf16 pattern b, the fp32 patterns (b << 16) + {0, 0x7fff, 0x8000, 0x8001, 0xffff}: the exact value, just below the tie,
    the tie, just above it, the top of the interval; uint32 [1280, 256]"""
    b = np.arange(65536, dtype=np.uint32) << 16
    return np.stack([b + o for o in (0, 0x7FFF, 0x8000, 0x8001, 0xFFFF)]).astype(np.uint32).reshape(1280, 256)


def f16_set():
    return np.arange(65536, dtype=np.uint16).reshape(256, 256)


def _torch_bits(t):
    import torch
    return t.view(torch.int16).numpy().view(np.uint16) if t.dtype == torch.bfloat16 else t.view(torch.int32).numpy().view(np.uint32)


def test_convert_f32_to_bf16_is_torch_on_the_full_set():
    import torch
    u = f32_set()
    subnormal = ((u & 0x7F800000) == 0) & ((u & 0x007FFFFF) != 0)
    assert int(subnormal.sum()) == 1278 and int(ref.is_nan(u).sum()) == 1278                           # the subnormal and the NaN inputs are in
    want = _torch_bits(torch.from_numpy(u.view(np.float32)).to(torch.bfloat16))
    got = ref.convert(u, "f32", "bf16")
    assert ref.diff(got, want) == []
    assert np.array_equal(ref.is_nan(got), ref.is_nan(u))                                              # NaN in, NaN out -- and nowhere else
    assert np.array_equal(got, ref.convert(u.view(np.float32), "f32", "bf16"))
    # synth's own rounding (what every fixture of the suite was made with) agrees, NaN included
    s = synth.f32_to_bf16_bits(u.view(np.float32))
    assert ref.diff(s, want) == [] and np.array_equal(ref.is_nan(s), ref.is_nan(u))
    # spot values: ties to even both ways, a subnormal kept, the largest finite value rounds to inf, inf and -0 stay
    for src, dst in ((0x3F808000, 0x3F80), (0x3F818000, 0x3F82), (0x00018000, 0x0002), (0x00008000, 0x0000), (0x00008001, 0x0001),
                     (0x7F7FFFFF, 0x7F80), (0x7F800000, 0x7F80), (0x80000000, 0x8000), (0xFF800000, 0xFF80)):
        assert int(ref.convert(np.array([[src]], np.uint32), "f32", "bf16")[0, 0]) == dst, hex(src)


def test_convert_f16_is_torch_on_all_patterns():
    import torch
    u = f16_set()
    t = torch.from_numpy(u.view(np.float16))
    f = ref.convert(u, "f16", "f32")
    assert ref.diff(f, _torch_bits(t.to(torch.float32))) == []
    assert np.array_equal(ref.is_nan(f), (u & 0x7FFF) > 0x7C00)
    # exact: back to f16 gives every non-NaN pattern again
    back = f.view(np.float32).astype(np.float16).view(np.uint16)
    assert np.array_equal(back[~ref.is_nan(f)], u[~ref.is_nan(f)])
    b = ref.convert(u, "f16", "bf16")
    assert ref.diff(b, _torch_bits(t.to(torch.bfloat16))) == []
    assert np.array_equal(ref.is_nan(b), (u & 0x7FFF) > 0x7C00)
    assert np.array_equal(b, ref.convert(f, "f32", "bf16"))                                            # one rounding, of the fp32 value


def test_convert_identities():
    u16, u32 = f16_set(), f32_set()
    same = ref.convert(u16, "bf16", "bf16")
    assert ref.diff(same, u16) == [] and np.array_equal(same[~ref.is_nan(u16)], u16[~ref.is_nan(u16)])   # (a signalling NaN comes out quiet)
    assert np.array_equal(ref.convert(u32, "f32", "f32"), u32)
    assert np.array_equal(ref.convert(u16, "bf16", "f32"), u16.astype(np.uint32) << 16)


def test_convert_slice_map():
    src = (np.arange(40 * 24, dtype=np.float32).reshape(40, 24) + 1)
    out = ref.convert_slice(src, "f32", 3, 8, 20, 16, "f32", 30, 20, dst_row0=5)
    assert np.array_equal(out[5:25, :16].view(np.float32), src[3:23, 8:24])
    assert (out[:5] == 0xFFFFFFFF).all() and (out[25:] == 0xFFFFFFFF).all() and (out[:, 16:] == 0xFFFFFFFF).all()
    g = ref.convert_slice(src, "f32", 0, 0, 40, 24, "f32", 96, 24, row_mode=1)
    u = ref.convert_slice(src, "f32", 0, 0, 40, 24, "f32", 96, 24, row_mode=2)
    assert np.array_equal(g[32:48].view(np.float32), src[16:32]) and np.array_equal(u[48:64].view(np.float32), src[16:32])
    assert np.array_equal(g[64:72].view(np.float32), src[32:40]) and (g[72:] == 0xFFFFFFFF).all() and (g[16:32] == 0xFFFFFFFF).all()
    hp = ref.convert_slice(src, "f32", 0, 0, 36, 24, "f32", 64, 24, head_pad=1, dm=12, d=16)
    assert np.array_equal(hp[16:22].view(np.float32), src[12:18]) and np.array_equal(hp[24:30].view(np.float32), src[18:24])
    assert (hp[22:24] == 0xFFFFFFFF).all() and (hp[30:32] == 0xFFFFFFFF).all()
    cp = ref.convert_slice(src, "f32", 0, 0, 40, 24, "f32", 40, 32, head_pad=2, dm=12, d=16)
    assert np.array_equal(cp[:, 24:30].view(np.float32), src[:, 18:24]) and (cp[:, 6:8] == 0xFFFFFFFF).all()


# ---- the images cover the sources ---------------------------------------------------------------------------------------------
def cfg_variant(name, **kw):
    c = dict(synth.CONFIGS[name])
    c.update(kw)
    return c


COVER = [("llama_a", {}, (1, 2)), ("qwen2_a", {}, (1, 2)), ("qwen2_a", dict(vocab_size=301), (1, 2)), ("llama_d100", {}, (1, 2)),
         ("mistral_d48", {}, (1, 2)), ("qwen2_d96", {}, (1, 2)), ("llama_tp4", {}, (1, 2, 4)), ("llama_a", dict(intermediate_size=360), (1, 2))]


def id_weights(cfg):
    """fp32 sources whose values are 1, 2, 3, ... in storage order: every element names itself (exact in fp32: the largest tensor has
    far fewer than 2^24 elements)"""
    return {name: (np.arange(int(np.prod(shape)), dtype=np.float32) + 1).reshape(shape) for name, shape in synth.tensor_shapes(cfg)}


@pytest.mark.parametrize("name,kw,tps", COVER, ids=["%s%s" % (n, "".join("-%s%s" % kv for kv in k.items())) for n, k, _ in COVER])
def test_images_cover_the_sources_exactly_once(name, kw, tps):
    cfg = cfg_variant(name, **kw)
    w = id_weights(cfg)
    D1 = ref.dims(cfg)
    for tie_lm_head in ((False, True) if cfg["family"] == "qwen2" else (False,)):
        ww = {k: v for k, v in w.items() if not (tie_lm_head and k == "lm_head.weight")}
        for tp in tps:
            imgs = [ref.model_image(cfg, ww, "f32", tp, r) for r in range(tp)]
            D = ref.dims(cfg, tp, 0)
            p = lambda l, s: "model.layers.%d.%s" % (l, s)       # noqa: E731
            ids = lambda key: np.concatenate([im[key].view(np.float32).ravel() for im in imgs])      # noqa: E731
            # shapes: what the layout description says
            nq = (D["Hs"] + 2 * D["Hkvs"]) * D["d"]
            im = imgs[0]
            assert im["embed"].shape == (D["V"], D["h"]) and im["lm_head"].shape == (D["Vs"], D["h"]) and im["norm"].shape == (D["h"], 1)
            for l in range(D["L"]):
                assert im["wqkv", l].shape == (nq, D["h"]) and im["wo", l].shape == (D["h"], D["Hs"] * D["d"])
                assert im["wgu", l].shape == (2 * D["Ip"], D["h"]) and im["wd", l].shape == (D["h"], D["Ip"])
                assert (("bqkv", l) in im) == D["bias"] and (not D["bias"] or im["bqkv", l].shape == (nq, 1))
            # sharded tensors: over the ranks every source element once, everything else zero
            for l in range(D["L"]):
                groups = [(("wqkv", l), [p(l, "self_attn.%s_proj.weight" % x) for x in "qkv"]), (("wo", l), [p(l, "self_attn.o_proj.weight")]),
                          (("wgu", l), [p(l, "mlp.gate_proj.weight"), p(l, "mlp.up_proj.weight")]), (("wd", l), [p(l, "mlp.down_proj.weight")])]
                if D["bias"]:
                    groups.append((("bqkv", l), [p(l, "self_attn.%s_proj.bias" % x) for x in "qkv"]))
                for key, names in groups:
                    got = ids(key)
                    n_src = sum(ww[n].size for n in names)
                    # (q, k and v -- gate and up -- number their elements from 1 each: compared as multisets; the order is checked below)
                    nz = got[got != 0]
                    assert nz.size == n_src, (key, tp)
                    want = np.sort(np.concatenate([ww[n].ravel() for n in names]))
                    assert np.array_equal(np.sort(nz), want), (key, tp)
                    assert got.size - nz.size == sum(i[key].size for i in imgs) - n_src                # the rest is padding, and it is zero
            # whole tensors on every rank; lm_head split by rows only when the vocabulary divides
            lm_src = ww.get("lm_head.weight", ww["model.embed_tokens.weight"])
            for r, im in enumerate(imgs):
                assert np.array_equal(im["embed"].view(np.float32), ww["model.embed_tokens.weight"])
                assert np.array_equal(im["norm"].view(np.float32).ravel(), ww["model.norm.weight"])
                for l in range(D["L"]):
                    assert np.array_equal(im["ln1", l].view(np.float32).ravel(), ww[p(l, "input_layernorm.weight")])
                    assert np.array_equal(im["ln2", l].view(np.float32).ravel(), ww[p(l, "post_attention_layernorm.weight")])
            if tp > 1 and D["V"] % tp == 0:
                assert np.array_equal(np.concatenate([i["lm_head"] for i in imgs]).view(np.float32), lm_src)
            else:
                assert all(np.array_equal(i["lm_head"].view(np.float32), lm_src) for i in imgs)
            # the order inside a shard: fused q | k | v by rank, heads in order, second halves d/2 apart from the first
            dm, d, Hs, Hkvs = D["dm"], D["d"], D["Hs"], D["Hkvs"]
            for r, im in enumerate(imgs):
                q = ww[p(0, "self_attn.q_proj.weight")]
                k = ww[p(0, "self_attn.k_proj.weight")]
                v = ww[p(0, "self_attn.v_proj.weight")]
                a = im["wqkv", 0].view(np.float32)
                assert np.array_equal(a[0], q[r * Hs * dm]) and np.array_equal(a[d // 2], q[r * Hs * dm + dm // 2])
                assert np.array_equal(a[Hs * d + d], k[(r * Hkvs + 1) * dm]) if Hkvs > 1 else True
                assert np.array_equal(a[(Hs + Hkvs) * d + d // 2 + dm // 2 - 1], v[r * Hkvs * dm + dm - 1])
                if dm != d:
                    assert not a[dm // 2:d // 2].any() and not a[d // 2 + dm // 2:d].any()
                o = im["wo", 0].view(np.float32)
                assert np.array_equal(o[:, d // 2], ww[p(0, "self_attn.o_proj.weight")][:, r * Hs * dm + dm // 2])
                gu = im["wgu", 0].view(np.float32)
                Is = D["Is"]
                assert np.array_equal(gu[17 + 16], ww[p(0, "mlp.gate_proj.weight")][r * Is + 17]) and np.array_equal(gu[16], ww[p(0, "mlp.up_proj.weight")][r * Is])
            assert D1["Ip"] % 16 == 0


def test_cover_set_has_the_hard_shapes():
    shapes = [ref.dims(cfg_variant(n, **k), tp) for n, k, tps in COVER for tp in tps]
    assert any(D["Is"] % 16 for D in shapes) and any(D["dm"] != D["d"] and D["d"] == 64 for D in shapes)
    assert any(D["dm"] == 100 for D in shapes) and any(D["dm"] == 96 and D["bias"] for D in shapes)
    assert any(D["V"] % 2 for D in shapes)


# ---- diff() sees what whole-model logits would not -------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sample():
    """llama_d100 (padded heads) with intermediate 360 (Is % 16 != 0 at tp 2), fp32 sources that are not bf16 values, bf16 images"""
    cfg = cfg_variant("llama_d100", intermediate_size=360)
    w = ref.rounding_sources(synth.synth_weights(cfg), "f32", "model.layers.0.self_attn.q_proj.weight")
    return cfg, w, ref.model_image(cfg, w, "bf16", 2, 0)


def test_diff_accepts_the_image_and_any_nan_for_a_nan(sample):
    cfg, w, img = sample
    for key, a in img.items():
        assert ref.diff(a.copy(), a) == [], key
    want = img["wqkv", 0].copy()
    want[0, :3] = (0x7FC0, 0xFFC1, 0x7F81)
    got = want.copy()
    got[0, :3] = (0xFFFF, 0x7FC0, 0x7FFF)
    assert ref.diff(got, want) == []                     # payload and sign of a NaN are not compared
    got[0, 1] = 0x7F80
    assert ref.diff(got, want)                           # ... but inf is no NaN
    got = want.copy()
    got[5, 5] = 0xFFFF
    assert ref.diff(got, want)                           # ... and a NaN where a number belongs (a poisoned element nobody wrote) shows
    assert ref.diff(img["norm"].view(np.float32), img["norm"]) == [] and ref.diff(img["wd", 0][:, :-1], img["wd", 0])


def test_diff_reports_each_subtle_mutation(sample):
    cfg, w, img = sample
    D = ref.dims(cfg, 2, 0)
    dm, d = D["dm"], D["d"]
    assert (dm, d, D["Is"], D["Ip"]) == (100, 128, 180, 192)
    # one element truncated instead of rounded
    src = w["model.layers.0.self_attn.q_proj.weight"]
    trunc = (src.view(np.uint32) >> 16).astype(np.uint16)
    want = img["wqkv", 0]
    r, c = np.argwhere(trunc[1:dm // 2] != want[1:dm // 2])[0] + (1, 0)           # (row 0 holds the special values)
    got = want.copy()
    got[r, c] = trunc[r, c]
    assert abs(int(got[r, c]) - int(want[r, c])) == 1 and len(ref.diff(got, want)) == 2
    # two rows swapped inside a 16-row gate/up group
    want = img["wgu", 1]
    got = want.copy()
    got[[3, 4]] = got[[4, 3]]
    assert ref.diff(got, want)
    # one nonzero padding element: between the halves of a head, behind Is in gate/up and in down
    for key, (r, c) in ((("wqkv", 0), (dm // 2, 7)), (("wo", 0), (7, d // 2 + dm // 2)), (("wgu", 0), (ref.gateup_row(D["Is"], 0), 9)),
                        (("wd", 1), (9, D["Is"]))):
        want = img[key]
        assert want[r, c] == 0
        got = want.copy()
        got[r, c] = 1                                    # the smallest bf16 subnormal: 9e-41
        assert ref.diff(got, want), key
    # a head's second half placed at dm/2 instead of d/2
    want = img["wqkv", 0]
    got = want.copy()
    got[dm // 2:dm] = want[d // 2:d // 2 + dm // 2]
    got[dm:d] = 0
    assert ref.diff(got, want)
    # the neighbouring rank's slice
    other = ref.model_image(cfg, w, "bf16", 2, 1)
    for key in (("wqkv", 0), ("wo", 0), ("wgu", 0), ("wd", 0), "lm_head"):
        assert ref.diff(other[key], img[key]), key
    assert ref.diff(other["embed"], img["embed"]) == []


def test_diff_reports_a_row_scale_left_at_its_pre_permutation_row():
    cfg = synth.CONFIGS["llama_a"]
    w = synth.synth_weights(cfg)
    img = ref.model_image(cfg, w, "bf16", 1, 0, e4m3=True)
    from test_w8_abi import quantize_rows_ref
    # scales computed on the HF row order of gate | up, then NOT moved with the rows
    gate = synth.bf16_bits_to_f32(w["model.layers.0.mlp.gate_proj.weight"])
    up = synth.bf16_bits_to_f32(w["model.layers.0.mlp.up_proj.weight"])
    _, s_hf = quantize_rows_ref(np.concatenate([gate, up]))
    want = img["wgu_s", 0]
    assert want.shape == (2 * 352, 1) and len(np.unique(want)) > 1
    got = s_hf.reshape(-1, 1).view(np.uint32)
    assert ref.diff(got, want)
    # ... while moved with the rows they are the image's
    Is = 352
    moved = np.zeros_like(got)
    for r in range(Is):
        moved[ref.gateup_row(r, 0)], moved[ref.gateup_row(r, 1)] = got[r], got[Is + r]
    assert ref.diff(moved, want) == []
    # the bf16 image is s * q exactly, and the e4m3 bytes are those of the final layout
    from test_w8_abi import dequantize
    back = dequantize(img["wgu_q", 0], want.view(np.float32).ravel())
    assert np.array_equal(ref.convert(back, "f32", "bf16"), img["wgu", 0]) and np.array_equal(ref.convert(img["wgu", 0], "bf16", "f32").view(np.float32), back)


# ---- the RoPE restatement --------------------------------------------------------------------------------------------------------
def test_rope_tables_restatement():
    for cfg in (synth.CONFIGS["llama_a"], synth.CONFIGS["llama_d100"], cfg_variant("qwen2_a", max_position_embeddings=32768)):
        D = ref.dims(cfg)
        cos, sin, bound, ang = ref.rope_tables(cfg)
        half, half_m = D["d"] // 2, D["dm"] // 2
        assert cos.shape == sin.shape == bound.shape == (D["max_pos"], half)
        assert (cos[0] == 1).all() and (sin[0] == 0).all() and (cos[:, half_m:] == 1).all() and (sin[:, half_m:] == 0).all()
        assert np.array_equal(ang[:, 0], np.arange(D["max_pos"], dtype=np.float64))                  # inv[0] is exactly 1
        assert (bound[0] == 0).all() and (bound[:, half_m:] == 0).all() and (bound[1:, 0] == 2.0 ** -23).all()
        assert np.array_equal(bound[1:, 1:half_m], 2.0 ** -23 + np.abs(ang[1:, 1:half_m]) * 2.0 ** -22)
        # the fp32 angle against the real one p * theta^(-2j/dm): the chain rounds the exponent (half an ulp of x <= 1, times ln(theta)
        # through the power), powf (1 ulp), the reciprocal and the product (half an ulp each)
        j = np.arange(half_m)
        exact = np.arange(D["max_pos"])[:, None] * float(np.float32(D["theta"])) ** (-2.0 * j / D["dm"])[None, :]
        assert (np.abs(ang[:, :half_m] - exact) <= np.abs(exact) * (np.log(D["theta"]) + 4) * 2.0 ** -24).all()
