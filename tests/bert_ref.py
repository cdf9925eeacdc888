"""CPU reference of the BERT / MiniLM encoder for the encoder tests: seeded synthetic weights and a numpy restatement of the forward
pass the library reproduces (include/fastllm_mi355x.h, "embeddings"):

  x = LN(word[ids] + pos[0..T) (+ token_type[0]))            eps 1e-12, whatever the config says
  per layer (post-LN):  a = softmax(Q K^T / sqrt(d)) V   (no mask);  x = LN(x + dense(a));  x = LN(x + out(gelu(inter(x))))
  gelu: tanh form (default) or erf form;  LN: mean and biased variance, (x - mean) / sqrt(var + eps) * w + b
  embedding = mean over the tokens of the last hidden states, divided by its L2 norm

ref_hidden / ref_embed run in fp64 by default; dtype=np.float32 runs every operation in float32 instead, which is how the tests
measure the noise floor of an fp32 execution (their bound is a multiple of |ref_float32 - ref_fp64|, never of the library's error).
Weights are drawn from np.random.RandomState and rounded to bf16 (as tests/synth.py does), so the fp64 reference, the fp32 mode
and the bf16 mode all start from the same values.
"""
import math
import zlib

import numpy as np

from synth import bf16_bits_to_f32, f32_to_bf16_bits

CONFIGS = {
    # head_dim 32 (MiniLM's), every size a power of two
    "bert_a": dict(hidden_size=128, num_attention_heads=4, intermediate_size=512, num_hidden_layers=2, vocab_size=200,
                   max_position_embeddings=64, layer_norm_eps=1e-12),
    # head_dim 64 (BERT-base's); I is not a multiple of 256 and h is not a power of two
    "bert_b": dict(hidden_size=192, num_attention_heads=3, intermediate_size=320, num_hidden_layers=2, vocab_size=300,
                   max_position_embeddings=160, layer_norm_eps=1e-5),
    # above the widths at which the row kernels take a second trip: a LayerNorm lane owns a second chunk from h = 520 on, a pooling
    # thread a second column from h = 257 on (all-MiniLM-L6 is 384 / 1536, BERT-base 768 / 3072).  head_dim 64, packed qkv rows of 1728.
    "bert_c": dict(hidden_size=576, num_attention_heads=9, intermediate_size=1088, num_hidden_layers=1, vocab_size=160,
                   max_position_embeddings=96, layer_norm_eps=1e-12),
}

# std of the intermediate.dense and token-type weights: large enough that the two GELU forms and the token-type option move the
# embedding by much more than the fp32 bound (tests/test_gpu_encoder.py, "options bite").  Measured on bert_a, T = 17 (seed below):
# fp32 bound 10 e32 + 1e-6 = 1.4e-6 (e32 = 4.4e-8); max |tanh - erf| = 2.0e-5 (13.6 x the bound), max |with - without token type| = 0.21.
STD = 0.05
STD_INTERMEDIATE = 0.15
STD_TOKEN_TYPE = 0.5


def tensor_shapes(cfg):
    h, i, V, P, L = (cfg["hidden_size"], cfg["intermediate_size"], cfg["vocab_size"], cfg["max_position_embeddings"],
                     cfg["num_hidden_layers"])
    out = [("embeddings.word_embeddings.weight", (V, h)), ("embeddings.position_embeddings.weight", (P, h)),
           ("embeddings.token_type_embeddings.weight", (2, h)), ("embeddings.LayerNorm.weight", (h,)), ("embeddings.LayerNorm.bias", (h,))]
    for l in range(L):
        p = "encoder.layer.%d." % l
        for nm, shape in (("attention.self.query", (h, h)), ("attention.self.key", (h, h)), ("attention.self.value", (h, h)),
                          ("attention.output.dense", (h, h)), ("intermediate.dense", (i, h)), ("output.dense", (h, i))):
            out += [(p + nm + ".weight", shape), (p + nm + ".bias", (shape[0],))]
        for nm in ("attention.output.LayerNorm", "output.LayerNorm"):
            out += [(p + nm + ".weight", (h,)), (p + nm + ".bias", (h,))]
    return out


def synth_weights(cfg, seed=0xBE27):
    """dict name -> uint16 array of bf16 bit patterns."""
    w = {}
    for name, shape in tensor_shapes(cfg):
        rs = np.random.RandomState((seed + zlib.crc32(name.encode())) & 0x7FFFFFFF)
        a = rs.standard_normal(shape).astype(np.float32)
        if name.endswith("LayerNorm.weight"):
            a = 1.0 + 0.1 * a
        elif name.endswith(".bias"):
            a = 0.1 * a
        elif "token_type" in name:
            a = STD_TOKEN_TYPE * a
        elif "intermediate.dense" in name:
            a = STD_INTERMEDIATE * a
        elif "embeddings." in name:
            a = 0.5 * a
        else:
            a = STD * a
        w[name] = f32_to_bf16_bits(a)
    return w


def as_f32(weights):
    return {k: bf16_bits_to_f32(v) for k, v in weights.items()}


def prompt_ids(cfg, T, seed=77):
    return np.random.RandomState(seed + T).randint(0, cfg["vocab_size"], size=T).astype(np.uint32)


_erf = np.vectorize(math.erf, otypes=[np.float64])


def gelu(v, activation):
    dt = v.dtype.type
    if activation == "gelu_erf":
        return dt(0.5) * v * (dt(1.0) + _erf(v.astype(np.float64) * math.sqrt(0.5)).astype(v.dtype))
    assert activation == "gelu_tanh"
    return dt(0.5) * v * (dt(1.0) + np.tanh(dt(math.sqrt(2.0 / math.pi)) * v * (dt(1.0) + dt(0.044715) * v * v)))


def layer_norm(x, w, b, eps):
    dt = x.dtype.type
    mean = x.mean(axis=-1, keepdims=True)
    var = ((x - mean) ** 2).mean(axis=-1, keepdims=True)
    return (x - mean) / np.sqrt(var + dt(eps)) * w + b


def attention(q, k, v, H):
    """unmasked softmax attention of one sequence: q / k / v [T, H*d] -> [T, H*d], in the arrays' dtype"""
    T, hd = q.shape
    d = hd // H
    dt = q.dtype.type
    out = np.empty_like(q)
    for hh in range(H):
        sl = slice(hh * d, (hh + 1) * d)
        s = q[:, sl] @ k[:, sl].T / dt(math.sqrt(d))
        s = s - s.max(axis=-1, keepdims=True)
        p = np.exp(s)
        p = p / p.sum(axis=-1, keepdims=True)
        out[:, sl] = p @ v[:, sl]
    return out


def ref_hidden(cfg, weights_f32, ids, dtype=np.float64, activation="gelu_tanh", add_token_type0=False):
    """last hidden states [T, h] of one sequence"""
    w = {k: v.astype(dtype) for k, v in weights_f32.items()}
    ids = np.asarray(ids, dtype=np.int64)
    T = ids.size
    assert 0 < T <= cfg["max_position_embeddings"]
    x = w["embeddings.word_embeddings.weight"][ids] + w["embeddings.position_embeddings.weight"][:T]
    if add_token_type0:
        x = x + w["embeddings.token_type_embeddings.weight"][0]
    x = layer_norm(x, w["embeddings.LayerNorm.weight"], w["embeddings.LayerNorm.bias"], 1e-12)
    eps = cfg["layer_norm_eps"]
    for l in range(cfg["num_hidden_layers"]):
        p = "encoder.layer.%d." % l
        lin = lambda nm, t: t @ w[p + nm + ".weight"].T + w[p + nm + ".bias"]      # noqa: E731
        a = attention(lin("attention.self.query", x), lin("attention.self.key", x), lin("attention.self.value", x),
                      cfg["num_attention_heads"])
        x = layer_norm(x + lin("attention.output.dense", a), w[p + "attention.output.LayerNorm.weight"],
                       w[p + "attention.output.LayerNorm.bias"], eps)
        x = layer_norm(x + lin("output.dense", gelu(lin("intermediate.dense", x), activation)), w[p + "output.LayerNorm.weight"],
                       w[p + "output.LayerNorm.bias"], eps)
    assert x.dtype == dtype
    return x


def pool(hidden):
    m = hidden.mean(axis=0)
    return m / np.sqrt((m * m).sum())


def ref_embed(cfg, weights_f32, ids, dtype=np.float64, **kw):
    """L2-normalised mean of the last hidden states, [h]"""
    return pool(ref_hidden(cfg, weights_f32, ids, dtype=dtype, **kw))
