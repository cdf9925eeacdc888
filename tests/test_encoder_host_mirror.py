"""The C++ host mirror of the reference's EmbeddingModel trait (fastllm::EmbeddingModel, fastllm_amd/host/fastllm_host.hpp) through
its C test surface: on the GPU embed_ids equals fl_encoder_embed and compute_similarity_ids is the cosine of embeddings.rs:22-37;
without a GPU (or on Device::Cpu) it refuses loudly."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import bert_ref as R

LIBDIR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "fastllm_amd", "lib")
NAME = "bert_a"


@pytest.fixture(scope="module")
def host():
    import fastllm_amd  # noqa: F401  (loads libfastllm_mi355x.so first)
    L = C.CDLL(os.path.join(LIBDIR, "libfastllm_host.so"))
    vp, sz = C.c_void_p, C.c_size_t
    L.flh_last_error.restype = C.c_char_p
    L.flh_embedding_create.argtypes = [C.c_char_p, vp, sz, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(vp)]
    L.flh_embedding_destroy.argtypes = [vp]
    L.flh_embedding_destroy.restype = None
    L.flh_embedding_size.argtypes = [vp]
    L.flh_embedding_size.restype = sz
    L.flh_embed_ids.argtypes = [vp, vp, sz, vp, C.POINTER(sz)]
    L.flh_embed_batch_ids.argtypes = [vp, vp, vp, sz, vp]
    L.flh_compute_similarity_ids.argtypes = [vp, vp, sz, vp, sz, C.POINTER(C.c_float)]
    return L


def create(host, device, with_vocab=True):
    from fastllm_amd import binding
    cfg = dict(R.CONFIGS[NAME])
    if not with_vocab:
        del cfg["vocab_size"]                       # the reference's BertConfig has none: the word-embedding table's rows count
    w = R.synth_weights(R.CONFIGS[NAME])
    arr, keep = binding._tensor_array(w)
    h = C.c_void_p()
    rc = host.flh_embedding_create(json.dumps(cfg).encode(), arr, len(w), 0, device, 0, 0, C.byref(h))
    return rc, h, w


def test_cpu_device_is_refused(host):
    rc, h, _ = create(host, -1)
    assert rc == -9 and b"no CPU path" in host.flh_last_error() and not h.value


@pytest.mark.gpu
def test_embed_ids_equals_the_c_abi_and_similarity_is_the_cosine(host):
    import fastllm_amd as fa
    cfg = R.CONFIGS[NAME]
    rc, h, w = create(host, 0, with_vocab=False)
    assert rc == 0, host.flh_last_error()
    assert host.flh_embedding_size(h) == cfg["hidden_size"]
    enc = fa.Encoder(cfg, w, dtype="f32")
    a, b = R.prompt_ids(cfg, 17), R.prompt_ids(cfg, 33)
    out = np.zeros(cfg["hidden_size"], np.float32)
    n = C.c_size_t(0)
    assert host.flh_embed_ids(h, a.ctypes.data, a.size, out.ctypes.data, C.byref(n)) == 0, host.flh_last_error()
    assert n.value == 17
    want = enc.embed([a, b])
    assert np.array_equal(out, enc.embed([a])[0])
    both = np.zeros((2, cfg["hidden_size"]), np.float32)
    ids, offs = np.concatenate([a, b]), np.array([0, 17, 50], np.uint64)
    assert host.flh_embed_batch_ids(h, ids.ctypes.data, offs.ctypes.data, 2, both.ctypes.data) == 0, host.flh_last_error()
    assert np.array_equal(both, want)

    def sim(x, y):
        s = C.c_float(0)
        assert host.flh_compute_similarity_ids(h, x.ctypes.data, x.size, y.ctypes.data, y.size, C.byref(s)) == 0, host.flh_last_error()
        return s.value

    assert abs(sim(a, a) - 1.0) <= 1e-6
    assert sim(a, b) == sim(b, a)
    ea, eb = (enc.embed([x])[0].astype(np.float64) for x in (a, b))
    assert abs(sim(a, b) - float(ea @ eb) / (np.linalg.norm(ea) * np.linalg.norm(eb))) <= 1e-6
    # an empty text: the library's error comes back through the mirror
    assert host.flh_embed_ids(h, a.ctypes.data, 0, out.ctypes.data, None) == -8
    host.flh_embedding_destroy(h)
    enc.close()
