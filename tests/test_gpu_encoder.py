"""The BERT / MiniLM encoder (fl_encoder_*) on the GPU against tests/bert_ref.py.

fp32 bound: NOT a constant.  For every case e32 = max |ref_float32 - ref_fp64| is measured on the CPU reference itself (bert_ref run
in numpy float32 against the same in fp64) and the library's fp32 mode must stay within 10 * e32 + 1e-6: the factor 10 covers the
different summation orders of the MFMA / tiled GEMMs and of the online softmax against numpy's.
bf16 bar: the project's own (tests/test_gpu_parity_bf16.py): || gpu_bf16 - ref64 || <= 1.5 || torch_bf16 - ref64 || + 1e-4, relative
L2, where torch_bf16 is an independent CPU torch bfloat16 execution of the same architecture (torch_bf16_hidden below)."""
import numpy as np
import pytest

import bert_ref as R

pytestmark = pytest.mark.gpu

RAGGED = [1, 17, 64, 3, 33, 16]
LENGTHS = {"bert_a": [1, 2, 15, 16, 17, 33, 64], "bert_b": [1, 2, 15, 16, 17, 33, 64, 65, 160], "bert_c": [1, 17, 65]}
CASES = [(n, T) for n in ("bert_a", "bert_b", "bert_c") for T in LENGTHS[n]]


@pytest.fixture(scope="module")
def fa():
    import fastllm_amd
    assert fastllm_amd.device_count() >= 1
    return fastllm_amd


_W, _REF, _ENC = {}, {}, {}


def weights(name):
    if name not in _W:
        w = R.synth_weights(R.CONFIGS[name])
        _W[name] = (w, R.as_f32(w))
    return _W[name]


def ref(name, ids, dtype=np.float64, **kw):
    """last hidden states of the CPU reference, computed once per case"""
    key = (name, tuple(int(i) for i in ids), np.dtype(dtype).name, tuple(sorted(kw.items())))
    if key not in _REF:
        h = R.ref_hidden(R.CONFIGS[name], weights(name)[1], ids, dtype=dtype, **kw)
        h.setflags(write=False)
        _REF[key] = h
    return _REF[key]


def bounds(name, ids, **kw):
    """(bound on hidden states, bound on embeddings) = 10 e32 + 1e-6, e32 from the reference's own float32 run"""
    h64, h32 = ref(name, ids, **kw), ref(name, ids, dtype=np.float32, **kw)
    eh = np.abs(h32 - h64).max()
    ee = np.abs(R.pool(h32) - R.pool(h64)).max()
    return 10 * eh + 1e-6, 10 * ee + 1e-6, eh, ee


@pytest.fixture(scope="module")
def encoder(fa):
    def get(name, dtype="f32", **kw):
        key = (name, dtype, tuple(sorted(kw.items())))
        if key not in _ENC:
            _ENC[key] = fa.Encoder(R.CONFIGS[name], weights(name)[0], dtype=dtype, **kw)
        return _ENC[key]
    yield get
    for e in _ENC.values():
        e.close()
    _ENC.clear()


def ragged_ids(name):
    return [R.prompt_ids(R.CONFIGS[name], T, seed=500 + i) for i, T in enumerate(RAGGED)]


# ---- fp32 parity ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,T", CASES)
def test_fp32_hidden_and_embedding(encoder, name, T):
    ids = R.prompt_ids(R.CONFIGS[name], T)
    bh, be, eh, ee = bounds(name, ids)
    enc = encoder(name)
    h = enc.hidden(ids)
    e = enc.embed([ids])[0]
    h64 = ref(name, ids)
    dh, de = np.abs(h - h64).max(), np.abs(e - R.pool(h64)).max()
    print("\n%s T=%d: hidden e32 %.3e achieved %.3e (bound %.3e); embedding e32 %.3e achieved %.3e (bound %.3e)" % (name, T, eh, dh, bh, ee, de, be))
    assert h.shape == (T, R.CONFIGS[name]["hidden_size"]) and np.isfinite(h).all()
    assert dh <= bh, (dh, bh)
    assert de <= be, (de, be)
    assert abs(np.linalg.norm(e.astype(np.float64)) - 1.0) <= 1e-5


def test_activation_and_token_type_options_bite(encoder):
    """Each option matches ITS reference within the fp32 bound, and the references are more than 4 bounds apart: a mix-up cannot pass."""
    name, ids = "bert_a", R.prompt_ids(R.CONFIGS["bert_a"], 17)
    base = R.pool(ref(name, ids))
    for kw in (dict(activation="gelu_erf"), dict(add_token_type0=True), dict(activation="gelu_erf", add_token_type0=True)):
        bh, be, eh, ee = bounds(name, ids, **kw)
        h64 = ref(name, ids, **kw)
        gap = np.abs(R.pool(h64) - base).max()
        assert gap > 4 * be, (kw, gap, be)                  # (the CPU precondition: bert_ref.py's weight scales are chosen for it)
        enc = encoder(name, **kw)
        dh, de = np.abs(enc.hidden(ids) - h64).max(), np.abs(enc.embed([ids])[0] - R.pool(h64)).max()
        print("\n%s: gap to the default %.3e; hidden %.3e (bound %.3e), embedding %.3e (bound %.3e)" % (kw, gap, dh, bh, de, be))
        assert dh <= bh and de <= be, (kw, dh, bh, de, be)
        assert np.abs(enc.embed([ids])[0] - base).max() > 2 * be          # and it is NOT the default's result


# ---- ragged batches ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["bert_a", "bert_b", "bert_c"])
def test_fp32_ragged_batch(encoder, name):
    seqs = ragged_ids(name)
    enc = encoder(name)
    got = enc.embed(seqs)
    for i, ids in enumerate(seqs):
        _, be, _, ee = bounds(name, ids)
        d_ref = np.abs(got[i] - R.pool(ref(name, ids))).max()
        d_alone = np.abs(got[i] - enc.embed([ids])[0]).max()
        print("\n%s row %d (T=%d): e32 %.3e, to the reference %.3e, to the sequence alone %.3e (bound %.3e)" % (name, i, len(ids), ee, d_ref, d_alone, be))
        assert d_ref <= be and d_alone <= be, (i, d_ref, d_alone, be)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("name", ["bert_a", "bert_b"])
def test_isolation_rows_do_not_depend_on_their_neighbours(fa, encoder, name, dtype):
    """The same batch with sequence 2 replaced by other ids of the same length: every other row is bit-identical (same kernels, same
    shapes, and no sum crosses a sequence).  First: two identical op_linear calls at the encoder's shapes are bit-identical."""
    cfg = R.CONFIGS[name]
    T, h, I = sum(RAGGED), cfg["hidden_size"], cfg["intermediate_size"]
    rs = np.random.RandomState(5)
    for N, K in ((3 * h, h), (h, h), (I, h), (h, I)):
        x, w = rs.standard_normal((T, K)).astype(np.float32), rs.standard_normal((N, K)).astype(np.float32)
        if dtype == "bf16":
            x, w = R.f32_to_bf16_bits(x), R.f32_to_bf16_bits(w)
        assert np.array_equal(fa.op_linear(x, w), fa.op_linear(x, w)), (N, K)
    seqs = ragged_ids(name)
    enc = encoder(name, dtype=dtype)
    a = enc.embed(seqs)
    other = list(seqs)
    other[2] = (seqs[2] + 1 + np.arange(seqs[2].size)) % cfg["vocab_size"]
    b = enc.embed(other)
    assert not np.array_equal(a[2], b[2])
    for i in (0, 1, 3, 4, 5):
        assert np.array_equal(a[i], b[i]), i
    assert np.array_equal(a, enc.embed(seqs))


# ---- bf16 -------------------------------------------------------------------------------------------------------------------------
def torch_bf16_hidden(name, ids):
    """an independent bfloat16 execution of the architecture: CPU torch, every tensor and every operation in torch.bfloat16"""
    import torch
    import torch.nn.functional as F
    key = ("torch", name, tuple(int(i) for i in ids))
    if key in _REF:
        return _REF[key]
    cfg = R.CONFIGS[name]
    w = {k: torch.from_numpy(v.copy()).to(torch.bfloat16) for k, v in weights(name)[1].items()}
    h, H = cfg["hidden_size"], cfg["num_attention_heads"]
    d, T = h // H, len(ids)
    idx = torch.from_numpy(np.asarray(ids, dtype=np.int64))
    x = w["embeddings.word_embeddings.weight"][idx] + w["embeddings.position_embeddings.weight"][:T]
    x = F.layer_norm(x, (h,), w["embeddings.LayerNorm.weight"], w["embeddings.LayerNorm.bias"], 1e-12)
    for l in range(cfg["num_hidden_layers"]):
        p = "encoder.layer.%d." % l
        lin = lambda nm, t: F.linear(t, w[p + nm + ".weight"], w[p + nm + ".bias"])      # noqa: E731
        q, k, v = (lin("attention.self." + n, x).view(T, H, d).transpose(0, 1) for n in ("query", "key", "value"))
        pr = torch.softmax(q @ k.transpose(1, 2) / (d ** 0.5), dim=-1)
        a = (pr @ v).transpose(0, 1).reshape(T, h)
        x = F.layer_norm(x + lin("attention.output.dense", a), (h,), w[p + "attention.output.LayerNorm.weight"],
                         w[p + "attention.output.LayerNorm.bias"], cfg["layer_norm_eps"])
        f = lin("output.dense", F.gelu(lin("intermediate.dense", x), approximate="tanh"))
        x = F.layer_norm(x + f, (h,), w[p + "output.LayerNorm.weight"], w[p + "output.LayerNorm.bias"], cfg["layer_norm_eps"])
    assert x.dtype == torch.bfloat16
    _REF[key] = x.to(torch.float32).numpy().astype(np.float64)
    return _REF[key]


def rel(a, b):
    return np.linalg.norm(a - b) / np.linalg.norm(b)


@pytest.mark.parametrize("name,T", [(n, T) for n in ("bert_a", "bert_b") for T in (1, 17, 64)] + [("bert_c", 17)])
def test_bf16_against_an_independent_bf16_execution(encoder, name, T):
    ids = R.prompt_ids(R.CONFIGS[name], T)
    h64, ht = ref(name, ids), torch_bf16_hidden(name, ids)
    enc = encoder(name, dtype="bf16")
    h, e = enc.hidden(ids), enc.embed([ids])[0]
    e64 = R.pool(h64)
    eg, et = rel(h, h64), rel(ht, h64)
    eeg, eet = rel(e, e64), rel(R.pool(ht), e64)
    print("\n%s T=%d bf16: hidden rel L2 gpu %.3e torch %.3e; embedding gpu %.3e torch %.3e; cosine to fp64 %.7f"
          % (name, T, eg, et, eeg, eet, float(e @ e64) / np.linalg.norm(e)))
    assert eg <= 1.5 * et + 1e-4, (eg, et)
    assert eeg <= 1.5 * eet + 1e-4, (eeg, eet)
    assert abs(np.linalg.norm(e.astype(np.float64)) - 1.0) <= 1e-5


@pytest.mark.parametrize("name", ["bert_a", "bert_b"])
def test_bf16_ragged_batch(encoder, name):
    seqs = ragged_ids(name)
    enc = encoder(name, dtype="bf16")
    got = enc.embed(seqs)
    for i, ids in enumerate(seqs):
        e64 = R.pool(ref(name, ids))
        bar = 1.5 * rel(R.pool(torch_bf16_hidden(name, ids)), e64) + 1e-4
        d_ref, d_alone = rel(got[i], e64), np.linalg.norm(got[i] - enc.embed([ids])[0]) / np.linalg.norm(e64)
        print("\n%s row %d (T=%d) bf16: to the reference %.3e, to the sequence alone %.3e (bar %.3e); cosine %.7f"
              % (name, i, len(ids), d_ref, d_alone, bar, float(got[i] @ e64) / np.linalg.norm(got[i])))
        assert d_ref <= bar and d_alone <= bar, (i, d_ref, d_alone, bar)


# ---- errors on the device path --------------------------------------------------------------------------------------------------
def test_call_errors_leave_the_encoder_usable(fa):
    name = "bert_a"
    cfg = R.CONFIGS[name]
    enc = fa.Encoder(cfg, weights(name)[0], dtype="f32", max_batch_tokens=32)
    ids = R.prompt_ids(cfg, 16)
    good = enc.embed([ids])

    def fails(code, fn):
        with pytest.raises(fa.FastLLMError) as e:
            fn()
        assert e.value.code == code, str(e.value)
        assert np.array_equal(enc.embed([ids]), good)       # still usable, same result

    fails(-8, lambda: enc.embed([ids, []]))                                    # an empty sequence
    fails(-8, lambda: enc.hidden([]))
    fails(-8, lambda: enc.hidden([1, cfg["vocab_size"], 2]))                   # id >= V
    fails(-7, lambda: enc.embed([list(ids), list(ids), [1]]))                  # 33 tokens > max_batch_tokens
    big = fa.Encoder(cfg, weights(name)[0], dtype="f32")
    with pytest.raises(fa.FastLLMError) as e:
        big.hidden(np.zeros(cfg["max_position_embeddings"] + 1, np.uint32))    # a sequence longer than P
    assert e.value.code == -7
    assert big.hidden(ids).shape == (16, cfg["hidden_size"])
    big.close()
    enc.close()


def test_missing_and_misshaped_tensors(fa):
    cfg = R.CONFIGS["bert_a"]
    w = dict(weights("bert_a")[0])
    del w["encoder.layer.1.output.dense.bias"]
    with pytest.raises(fa.FastLLMError) as e:
        fa.Encoder(cfg, w)
    assert e.value.code == -2 and "encoder.layer.1.output.dense.bias" in str(e.value)
    w = dict(weights("bert_a")[0])
    w["encoder.layer.0.intermediate.dense.weight"] = w["encoder.layer.0.intermediate.dense.weight"][:, :-8]
    with pytest.raises(fa.FastLLMError) as e:
        fa.Encoder(cfg, w)
    assert e.value.code == -3
    w = dict(weights("bert_a")[0])
    del w["embeddings.token_type_embeddings.weight"]
    fa.Encoder(cfg, w).close()                              # not needed as the reference runs ...
    with pytest.raises(fa.FastLLMError) as e:
        fa.Encoder(cfg, w, add_token_type0=True)            # ... but it is with the HF option
    assert e.value.code == -2
