"""ctypes binding of include/fastllm_mi355x.h (harness only; no arithmetic here).

Loading fails loudly when the HIP library has not been built: there is no fallback path.
"""
import collections
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("FL_LIB_PATH") or os.path.join(_HERE, "lib", "libfastllm_mi355x.so")   # FL_LIB_PATH: kernel-variant experiments

FAMILY = {"llama": 0, "mistral": 1, "qwen2": 2}
F32, BF16, F16 = 0, 1, 2
TP_NONE, TP_SINGLE_PROCESS, TP_MULTI_PROCESS, TP_EMULATED = 0, 1, 2, 3
UNIQUE_ID_BYTES = 128
IPC_HANDLE_BYTES = 64
WEIGHTS_COMPUTE_DTYPE, WEIGHTS_E4M3_ROW = 0, 1
DECODE_WEIGHTS = {None: WEIGHTS_COMPUTE_DTYPE, "compute": WEIGHTS_COMPUTE_DTYPE, "e4m3": WEIGHTS_E4M3_ROW}


class FastLLMError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("fastllm_mi355x error %d: %s" % (code, msg))
        self.code = code


class FlConfig(C.Structure):
    _fields_ = [("family", C.c_int32), ("qkv_bias", C.c_int32), ("hidden_size", C.c_int64),
                ("intermediate_size", C.c_int64), ("vocab_size", C.c_int64), ("num_hidden_layers", C.c_int64),
                ("num_attention_heads", C.c_int64), ("num_key_value_heads", C.c_int64),
                ("max_position_embeddings", C.c_int64), ("sliding_window", C.c_int64),
                ("rms_norm_eps", C.c_double), ("rope_theta", C.c_double)]


class FlTensor(C.Structure):
    _fields_ = [("name", C.c_char_p), ("dtype", C.c_int32), ("ndim", C.c_int32), ("shape", C.c_int64 * 4),
                ("data", C.c_void_p), ("device", C.c_int32), ("_pad", C.c_int32)]


class FlParallel(C.Structure):
    _fields_ = [("mode", C.c_int32), ("tp_size", C.c_int32), ("tp_rank", C.c_int32), ("n_device_ids", C.c_int32),
                ("device_ids", C.POINTER(C.c_int32)), ("unique_id", C.c_void_p)]


class FlModelInfo(C.Structure):
    _fields_ = [("cfg", FlConfig), ("head_dim", C.c_int64), ("compute_dtype", C.c_int32), ("tp_size", C.c_int32),
                ("weight_bytes_per_token", C.c_int64), ("kv_bytes_per_position", C.c_int64),
                ("hbm_bytes_allocated", C.c_int64), ("small_collectives", C.c_int32), ("fused_all_reduce", C.c_int32),
                ("rccl_ranks", C.c_int32), ("decode_weights", C.c_int32)]


class FlModelOptions(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("decode_weights", C.c_int32), ("_reserved", C.c_int64 * 3)]


class FlSampling(C.Structure):
    _fields_ = [("temperature", C.c_double), ("seed", C.c_uint64), ("draws_done", C.c_uint64)]


class FlSampler(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("top_k", C.c_int32), ("temperature", C.c_double), ("top_p", C.c_double),
                ("seed", C.c_uint64), ("draws_done", C.c_uint64), ("_reserved", C.c_int64 * 2)]


def make_sampler(temperature, seed=0, draws_done=0, top_p=None, top_k=None):
    """fl_sampler: top_p None (or outside (0, 1)) and top_k None (or 0) are off."""
    return FlSampler(C.sizeof(FlSampler), 0 if top_k is None else int(top_k), temperature, 0.0 if top_p is None else top_p,
                     seed, draws_done)


LOGPROBS_MAX_TOP = 20


class FlLogprobs(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("top_n", C.c_int32), ("token_logprob", C.c_void_p), ("top_ids", C.c_void_p),
                ("top_logprobs", C.c_void_p), ("_reserved", C.c_int64 * 2)]


class _LogprobArrays:
    """Host arrays of one fl_logprobs: n rows of top_n entries (the arrays stay alive as long as this object does)."""

    def __init__(self, n, top_n):
        self.top_n = int(top_n)
        w = max(self.top_n, 0)
        self.token = np.zeros(max(n, 1), dtype=np.float32)
        self.ids = np.zeros((max(n, 1), w), dtype=np.uint32)
        self.lps = np.zeros((max(n, 1), w), dtype=np.float32)

    def struct(self):
        return FlLogprobs(C.sizeof(FlLogprobs), self.top_n, self.token.ctypes.data, self.ids.ctypes.data if self.top_n > 0 else None,
                          self.lps.ctypes.data if self.top_n > 0 else None)

    def cut(self, n):
        return self.token[:n], self.ids[:n], self.lps[:n]


class FlScore(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("top_n", C.c_int32), ("targets", C.c_void_p), ("target_logprob", C.c_void_p),
                ("target_rank", C.c_void_p), ("top_ids", C.c_void_p), ("top_logprobs", C.c_void_p), ("logits_out", C.c_void_p),
                ("_reserved", C.c_int64 * 2)]


SCORE_NO_TARGET = 0xFFFFFFFF
# one scoring call's result: target_logprob float32 [T] (NaN: no target), target_rank uint32 [T] (0: no target), top_ids uint32
# [T, top_n], top_logprobs float32 [T, top_n], logits float32 [T, V] or None
ScoreResult = collections.namedtuple("ScoreResult", ["target_logprob", "target_rank", "top_ids", "top_logprobs", "logits"])


class _ScoreArrays:
    """Host arrays of one fl_score over T rows (they stay alive as long as this object does)."""

    def __init__(self, T, top_n, targets=None, V=None):
        self.T, self.top_n = int(T), int(top_n)
        w = max(self.top_n, 0)
        self.targets = None if targets is None else np.ascontiguousarray(targets, dtype=np.uint32).reshape(-1)
        assert self.targets is None or self.targets.size == self.T
        self.lp = np.zeros(max(self.T, 1), dtype=np.float32)
        self.rank = np.zeros(max(self.T, 1), dtype=np.uint32)
        self.ids = np.zeros((max(self.T, 1), w), dtype=np.uint32)
        self.lps = np.zeros((max(self.T, 1), w), dtype=np.float32)
        self.logits = None if V is None else np.empty((max(self.T, 1), V), dtype=np.float32)

    def struct(self):
        return FlScore(C.sizeof(FlScore), self.top_n, None if self.targets is None else self.targets.ctypes.data, self.lp.ctypes.data,
                       self.rank.ctypes.data, self.ids.ctypes.data if self.top_n > 0 else None,
                       self.lps.ctypes.data if self.top_n > 0 else None, None if self.logits is None else self.logits.ctypes.data)

    def result(self):
        T = self.T
        return ScoreResult(self.lp[:T], self.rank[:T], self.ids[:T], self.lps[:T], None if self.logits is None else self.logits[:T])


class FlLogitRules(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("n_bias", C.c_uint32), ("bias_ids", C.c_void_p), ("bias_values", C.c_void_p),
                ("repetition_penalty", C.c_float), ("frequency_penalty", C.c_float), ("presence_penalty", C.c_float),
                ("_reserved", C.c_int64 * 2)]


def make_logit_rules(logit_bias=None, repetition_penalty=1.0, frequency_penalty=0.0, presence_penalty=0.0):
    """fl_logit_rules from a {id: bias} mapping (or a list of pairs) and the three penalties; returns (struct, arrays to keep alive)."""
    pairs = list(logit_bias.items()) if hasattr(logit_bias, "items") else list(logit_bias or ())
    ids = np.ascontiguousarray([p[0] for p in pairs], dtype=np.uint32)
    vals = np.ascontiguousarray([p[1] for p in pairs], dtype=np.float32)
    st = FlLogitRules(C.sizeof(FlLogitRules), len(pairs), ids.ctypes.data if len(pairs) else None, vals.ctypes.data if len(pairs) else None,
                      repetition_penalty, frequency_penalty, presence_penalty)
    return st, (ids, vals)


class FlGuideDesc(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("n_states", C.c_uint32), ("row_ptr", C.c_void_p), ("tokens", C.c_void_p),
                ("next", C.c_void_p), ("_reserved", C.c_int64 * 2)]


class FlNormLinearArgs(C.Structure):
    _fields_ = [("struct_size", C.c_size_t), ("form", C.c_int32), ("dtype", C.c_int32), ("epilogue", C.c_int32), ("pro", C.c_int32),
                ("T", C.c_int64), ("N", C.c_int64), ("K", C.c_int64), ("x_res", C.c_void_p), ("x", C.c_void_p), ("delta", C.c_void_p),
                ("norm_w", C.c_void_p), ("embed", C.c_void_p), ("tokens", C.c_void_p), ("w", C.c_void_p), ("w_scale", C.c_void_p),
                ("bias", C.c_void_p), ("vocab", C.c_int64), ("n_slab", C.c_int32), ("repeat", C.c_int32), ("eps", C.c_float),
                ("reserved", C.c_float), ("y", C.c_void_p), ("x_out", C.c_void_p), ("kernels_out", C.c_void_p)]


class FlLinearResidArgs(C.Structure):
    _fields_ = [("struct_size", C.c_size_t), ("T", C.c_int64), ("N", C.c_int64), ("K", C.c_int64), ("N2", C.c_int64), ("x", C.c_void_p),
                ("w", C.c_void_p), ("bias", C.c_void_p), ("h_in", C.c_void_p), ("w_next", C.c_void_p), ("w2", C.c_void_p),
                ("eps", C.c_float), ("lazy", C.c_int32), ("epi2", C.c_int32), ("repeat", C.c_int32), ("h_out", C.c_void_p),
                ("xn_out", C.c_void_p), ("inv_rms_out", C.c_void_p), ("part_out", C.c_void_p), ("y2_out", C.c_void_p),
                ("kernels_out", C.c_void_p)]


class FlGemvResidArgs(C.Structure):
    _fields_ = [("struct_size", C.c_size_t), ("mode", C.c_int32), ("epi2", C.c_int32), ("repeat", C.c_int32), ("reserved", C.c_int32),
                ("N", C.c_int64), ("K", C.c_int64), ("N2", C.c_int64), ("H", C.c_int64), ("Hkv", C.c_int64), ("d", C.c_int64),
                ("max_pos", C.c_int64), ("pos", C.c_int64), ("len", C.c_int64), ("seq_alloc", C.c_int64), ("x", C.c_void_p), ("w", C.c_void_p),
                ("h_in", C.c_void_p), ("w_next", C.c_void_p), ("xs", C.c_void_p), ("cs", C.c_void_p), ("w2", C.c_void_p), ("cos_tab", C.c_void_p),
                ("sin_tab", C.c_void_p), ("eps", C.c_float), ("reserved2", C.c_float), ("h_out", C.c_void_p), ("xs_out", C.c_void_p),
                ("cs_out", C.c_void_p), ("delta_out", C.c_void_p), ("y_out", C.c_void_p), ("inv_out", C.c_void_p), ("h_ref", C.c_void_p),
                ("y_ref", C.c_void_p), ("inv_ref", C.c_void_p), ("amax_out", C.c_void_p)]


class FlRopeSeqs(C.Structure):
    _fields_ = [("n_seq", C.c_int32), ("layers", C.c_int32), ("layer", C.c_int32), ("reserved", C.c_int32), ("count", C.c_void_p),
                ("pos", C.c_void_p), ("len", C.c_void_p), ("seq_alloc", C.c_void_p), ("v_transposed", C.c_void_p), ("k_cache", C.c_void_p),
                ("v_cache", C.c_void_p)]


class FlRopeKvArgs(C.Structure):
    _fields_ = [("struct_size", C.c_size_t), ("form", C.c_int32), ("dtype", C.c_int32), ("n_slab", C.c_int32), ("repeat", C.c_int32),
                ("H", C.c_int64), ("Hkv", C.c_int64), ("d", C.c_int64), ("max_pos", C.c_int64), ("qkv", C.c_void_p), ("bias", C.c_void_p),
                ("cos_tab", C.c_void_p), ("sin_tab", C.c_void_p), ("seqs", FlRopeSeqs), ("q_out", C.c_void_p), ("kernels_out", C.c_void_p)]


class FlQkvRopeArgs(C.Structure):
    _fields_ = [("struct_size", C.c_size_t), ("form", C.c_int32), ("dtype", C.c_int32), ("n_slab", C.c_int32), ("repeat", C.c_int32),
                ("T", C.c_int64), ("K", C.c_int64), ("H", C.c_int64), ("Hkv", C.c_int64), ("d", C.c_int64), ("max_pos", C.c_int64),
                ("vocab", C.c_int64), ("x_res", C.c_void_p), ("delta", C.c_void_p), ("norm_w", C.c_void_p), ("embed", C.c_void_p),
                ("tokens", C.c_void_p), ("w", C.c_void_p), ("w_scale", C.c_void_p), ("bias", C.c_void_p), ("cos_tab", C.c_void_p),
                ("sin_tab", C.c_void_p), ("eps", C.c_float), ("reserved", C.c_float), ("seqs", FlRopeSeqs), ("q_out", C.c_void_p),
                ("x_out", C.c_void_p), ("kernels_out", C.c_void_p)]


class FlAttnOprojRepArgs(C.Structure):
    _fields_ = [("struct_size", C.c_size_t), ("H", C.c_int64), ("Hkv", C.c_int64), ("d", C.c_int64), ("N", C.c_int64), ("s_past", C.c_int64),
                ("k_rows", C.c_int64), ("capacity", C.c_int64), ("q", C.c_void_p), ("k", C.c_void_p), ("v", C.c_void_p), ("w_o", C.c_void_p),
                ("pad_value", C.c_float), ("repeat", C.c_int32), ("query_only", C.c_int32), ("reserved", C.c_int32), ("out", C.c_void_p),
                ("info_out", C.c_void_p)]


class FlEncoderRowsArgs(C.Structure):
    _fields_ = [("struct_size", C.c_size_t), ("form", C.c_int32), ("dtype", C.c_int32), ("n_slab", C.c_int32), ("repeat", C.c_int32),
                ("act", C.c_int32), ("reserved", C.c_int32), ("T", C.c_int64), ("h", C.c_int64), ("vocab", C.c_int64), ("P", C.c_int64),
                ("n_seq", C.c_size_t), ("word", C.c_void_p), ("pos", C.c_void_p), ("tt0", C.c_void_p), ("ids", C.c_void_p),
                ("offsets", C.c_void_p), ("x", C.c_void_p), ("slabs", C.c_void_p), ("bias", C.c_void_p), ("ln_w", C.c_void_p),
                ("ln_b", C.c_void_p), ("eps", C.c_float), ("reserved2", C.c_float), ("x_res_out", C.c_void_p), ("out", C.c_void_p)]


class FlConvertSliceArgs(C.Structure):
    _fields_ = [("struct_size", C.c_size_t), ("src_dtype", C.c_int32), ("dst_dtype", C.c_int32), ("row_mode", C.c_int32),
                ("head_pad", C.c_int32), ("via_bf16", C.c_int32), ("reserved", C.c_int32), ("R", C.c_int64), ("C", C.c_int64),
                ("r0", C.c_int64), ("c0", C.c_int64), ("rows", C.c_int64), ("cols", C.c_int64), ("dst_rows", C.c_int64), ("dst_ld", C.c_int64), ("dst_row0", C.c_int64), ("dm", C.c_int64),
                ("d", C.c_int64), ("src", C.c_void_p), ("dst", C.c_void_p)]


# selectors of Model.tensor (FL_MT_* of the header); ELEM_E4M3: the element code of the *_q tensors
MODEL_TENSORS = {"embed": 0, "norm": 1, "lm_head": 2, "cos_tab": 3, "sin_tab": 4, "wqkv": 5, "bqkv": 6, "wo": 7, "wgu": 8, "wd": 9, "ln1": 10,
                 "ln2": 11, "wqkv_q": 12, "wqkv_s": 13, "wo_q": 14, "wo_s": 15, "wgu_q": 16, "wgu_s": 17, "wd_q": 18, "wd_s": 19,
                 "lm_head_q": 20, "lm_head_s": 21}
ELEM_E4M3 = 3

# act of op_encoder_bias_act
ENC_ACT = {None: -1, "none": -1, "gelu_tanh": 0, "gelu_erf": 1}

# kernels_out[0] of op_rope_kv
ROPE_KV_NAMES = ("scalar", "vector", "batch", "packed")

# kernel codes in the kernels_out arrays of op_norm_linear / op_linear_resid (FL_LK_* of the header)
LK_NAMES = ("none", "gemv", "h4", "w14", "skf", "dma", "skinny", "8p", "8p_streamk", "256", "128", "4w_rope", "generic", "f32_rows", "f32_mfma")


def make_guide_desc(row_ptr, tokens, next):
    """fl_guide_desc from the CSR arrays of a token-level automaton; returns (struct, arrays to keep alive)."""
    rp = np.ascontiguousarray(row_ptr, dtype=np.uint64).reshape(-1)
    tk = np.ascontiguousarray(tokens, dtype=np.uint32).reshape(-1)
    nx = np.ascontiguousarray(next, dtype=np.uint32).reshape(-1)
    assert rp.size >= 1 and tk.size == nx.size
    st = FlGuideDesc(C.sizeof(FlGuideDesc), rp.size - 1, rp.ctypes.data, tk.ctypes.data if tk.size else None, nx.ctypes.data if nx.size else None)
    return st, (rp, tk, nx)


class FlEmbed(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("pooling", C.c_int32), ("mask", C.c_int32), ("normalize", C.c_int32),
                ("dimensions", C.c_int64), ("_reserved", C.c_int64 * 2)]


POOLING = {"last": 0, "mean": 1, "first": 2, "none": 3}
ATTN_MASK = {"causal": 0, "full": 1}


def make_embed(pooling="last", mask="causal", normalize=True, dimensions=0):
    """fl_embed; pooling / mask by name (POOLING, ATTN_MASK) or by their integer codes."""
    return FlEmbed(C.sizeof(FlEmbed), pooling if isinstance(pooling, int) else POOLING[pooling],
                   mask if isinstance(mask, int) else ATTN_MASK[mask], int(normalize), int(dimensions))


class FlLookup(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("max_draft", C.c_int32), ("ngram_max", C.c_int32), ("ngram_min", C.c_int32),
                ("_pad", C.c_int32), ("_reserved", C.c_int64 * 2)]


class FlSpecStats(C.Structure):
    _fields_ = [("steps", C.c_uint64), ("drafted", C.c_uint64), ("accepted", C.c_uint64)]


VERIFY_MAX_DRAFT = 15


def make_lookup(max_draft=7, ngram_max=3, ngram_min=1):
    return FlLookup(C.sizeof(FlLookup), int(max_draft), int(ngram_max), int(ngram_min))


class FlEncoderConfig(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("activation", C.c_int32), ("add_token_type0", C.c_int32), ("_pad", C.c_int32),
                ("hidden_size", C.c_int64), ("intermediate_size", C.c_int64), ("num_hidden_layers", C.c_int64),
                ("num_attention_heads", C.c_int64), ("max_position_embeddings", C.c_int64), ("vocab_size", C.c_int64),
                ("max_batch_tokens", C.c_int64), ("layer_norm_eps", C.c_double), ("_reserved", C.c_int64 * 2)]


ACTIVATION = {"gelu_tanh": 0, "gelu": 0, "gelu_erf": 1}


def make_encoder_config(cfg, activation="gelu_tanh", add_token_type0=False, max_batch_tokens=0):
    """fl_encoder_config from a BERT config dict (the fields of the reference's BertConfig + vocab_size)."""
    c = FlEncoderConfig()
    c.struct_size = C.sizeof(FlEncoderConfig)
    c.activation = activation if isinstance(activation, int) else ACTIVATION[activation]
    c.add_token_type0 = int(bool(add_token_type0))
    c.hidden_size = cfg["hidden_size"]
    c.intermediate_size = cfg["intermediate_size"]
    c.num_hidden_layers = cfg["num_hidden_layers"]
    c.num_attention_heads = cfg["num_attention_heads"]
    c.max_position_embeddings = cfg["max_position_embeddings"]
    c.vocab_size = cfg["vocab_size"]
    c.max_batch_tokens = int(max_batch_tokens)
    c.layer_norm_eps = cfg["layer_norm_eps"]
    return c


class FlKernelStat(C.Structure):
    _fields_ = [("name", C.c_char * 48), ("launches", C.c_int64), ("total_ms", C.c_double), ("bytes", C.c_double),
                ("flops", C.c_double)]


_LIB = None


def lib():
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError("%s is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                              "(there is no CPU fallback)" % LIB_PATH)
        L = C.CDLL(LIB_PATH)
        vp, sz = C.c_void_p, C.c_size_t
        L.fl_abi_version.restype = C.c_int
        L.fl_last_error.restype = C.c_char_p
        L.fl_device_count.argtypes = [C.POINTER(C.c_int)]
        L.fl_comm_unique_id.argtypes = [vp]
        L.fl_comm_ipc_export.argtypes = [vp, vp]
        L.fl_comm_ipc_connect.argtypes = [vp, vp]
        L.fl_model_create.argtypes = [C.POINTER(FlConfig), C.POINTER(FlTensor), sz, C.c_int32, C.POINTER(FlParallel), C.POINTER(vp)]
        L.fl_model_create_opts.argtypes = [C.POINTER(FlConfig), C.POINTER(FlTensor), sz, C.c_int32, C.POINTER(FlParallel),
                                           C.POINTER(FlModelOptions), C.POINTER(vp)]
        L.fl_model_retain.argtypes = [vp]
        L.fl_model_retain.restype = None
        L.fl_model_release.argtypes = [vp]
        L.fl_model_release.restype = None
        L.fl_model_get_info.argtypes = [vp, C.POINTER(FlModelInfo)]
        L.fl_cache_create.argtypes = [vp, sz, C.POINTER(vp)]
        L.fl_cache_reset.argtypes = [vp]
        L.fl_cache_reset.restype = None
        L.fl_cache_len.argtypes = [vp]
        L.fl_cache_len.restype = sz
        L.fl_cache_capacity.argtypes = [vp]
        L.fl_cache_capacity.restype = sz
        L.fl_cache_destroy.argtypes = [vp]
        L.fl_cache_destroy.restype = None
        L.fl_forward.argtypes = [vp, vp, vp, sz, sz, vp]
        L.fl_forward_argmax.argtypes = [vp, vp, vp, sz, sz, vp]
        L.fl_decode_greedy.argtypes = [vp, vp, C.c_uint32, sz, sz, C.c_int64, vp, C.POINTER(sz)]
        L.fl_forward_sample.argtypes = [vp, vp, vp, sz, sz, C.POINTER(FlSampling), vp]
        L.fl_decode_sample.argtypes = [vp, vp, C.c_uint32, sz, sz, C.c_int64, C.POINTER(FlSampling), vp, C.POINTER(sz)]
        L.fl_op_sample.argtypes = [vp, C.c_int64, C.POINTER(FlSampling), C.c_int64, vp]
        L.fl_forward_sample_ex.argtypes = [vp, vp, vp, sz, sz, C.POINTER(FlSampler), vp]
        L.fl_decode_sample_ex.argtypes = [vp, vp, C.c_uint32, sz, sz, C.c_int64, C.POINTER(FlSampler), vp, C.POINTER(sz)]
        L.fl_op_sample_ex.argtypes = [vp, C.c_int64, C.POINTER(FlSampler), C.c_int64, vp, vp]
        L.fl_batch_decode_each_ex.argtypes = [vp, vp, vp, C.c_size_t, vp, vp, vp, vp]
        L.fl_forward_sample_lp.argtypes = [vp, vp, vp, sz, sz, C.POINTER(FlSampler), vp, C.POINTER(FlLogprobs)]
        L.fl_decode_sample_lp.argtypes = [vp, vp, C.c_uint32, sz, sz, C.c_int64, C.POINTER(FlSampler), vp, C.POINTER(sz), C.POINTER(FlLogprobs)]
        L.fl_batch_decode_each_lp.argtypes = [vp, vp, vp, C.c_size_t, vp, vp, vp, vp, vp]
        L.fl_op_logprobs.argtypes = [vp, C.c_int64, C.c_int64, vp, C.c_int32, vp, vp, vp]
        L.fl_forward_score.argtypes = [vp, vp, vp, sz, sz, C.POINTER(FlScore)]
        L.fl_batch_score.argtypes = [vp, vp, sz, vp, vp, vp, C.POINTER(FlScore)]
        L.fl_op_score.argtypes = [vp, C.c_int64, C.c_int64, vp, C.c_int32, vp, vp, vp, vp]
        L.fl_op_score_time.argtypes = [vp, C.c_int64, C.c_int64, vp, C.c_int32, C.c_int32, C.POINTER(C.c_double)]
        L.fl_cache_set_logit_rules.argtypes = [vp, vp, C.POINTER(FlLogitRules), vp, sz, vp, sz]
        L.fl_cache_logit_counts.argtypes = [vp, vp, vp]
        L.fl_op_logit_rules.argtypes = [vp, C.c_int64, C.c_int64, vp, vp, vp, vp, C.c_int32, vp, vp]
        L.fl_guide_create.argtypes = [vp, C.POINTER(FlGuideDesc), C.POINTER(vp)]
        L.fl_guide_destroy.argtypes = [vp]
        L.fl_guide_destroy.restype = None
        L.fl_cache_set_guide.argtypes = [vp, vp, vp, C.c_uint32]
        L.fl_cache_guide_state.argtypes = [vp, C.POINTER(C.c_uint32)]
        L.fl_op_guide_mask.argtypes = [vp, C.c_int64, C.c_int64, C.POINTER(FlGuideDesc), vp, vp, vp, vp, vp]
        L.fl_op_attention.argtypes = [vp, vp, vp, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_int32, C.c_int32, vp]
        L.fl_op_attention_plain.argtypes = [vp, vp, vp, C.c_int32, C.c_int32, C.c_int32] + [C.c_int64] * 9 + [C.c_int32, C.c_float, C.c_int32, vp]
        L.fl_op_attention_batch.argtypes = [vp, vp, vp, C.c_int32, C.c_int32, C.c_int64, vp, vp, vp, vp] + [C.c_int64] * 5 + [C.c_float, C.c_int32, vp]
        L.fl_op_attention_packed.argtypes = [vp, vp, vp, C.c_int64, vp, vp, vp, vp] + [C.c_int64] * 6 + [C.c_float, vp]
        L.fl_op_attention_packed_ex.argtypes = [vp, vp, vp, C.c_int64, vp, vp, vp, vp] + [C.c_int64] * 6 + [C.c_float, C.c_int32, vp]
        L.fl_batch_prefill.argtypes = [vp, vp, sz, vp, vp, vp, vp, vp, vp]
        L.fl_batch_embed.argtypes = [vp, vp, sz, vp, vp, vp, C.POINTER(FlEmbed), vp]
        L.fl_op_pool_rows.argtypes = [vp, vp, vp, vp, sz, C.c_int64, C.POINTER(FlEmbed), vp]
        L.fl_op_pool_rows_time.argtypes = [vp, vp, vp, vp, sz, C.c_int64, C.POINTER(FlEmbed), C.c_int32, C.POINTER(C.c_double)]
        L.fl_batch_create.argtypes = [vp, vp, sz, C.POINTER(vp)]
        L.fl_batch_destroy.argtypes = [vp]
        L.fl_batch_destroy.restype = None
        L.fl_batch_replace.argtypes = [vp, C.c_size_t, vp]
        L.fl_batch_decode_each.argtypes = [vp, vp, vp, C.c_size_t, vp, vp, vp, vp]
        L.fl_batch_forward.argtypes = [vp, vp, vp, vp, vp]
        L.fl_batch_decode.argtypes = [vp, vp, vp, sz, C.c_int64, C.POINTER(FlSampling), vp, vp]
        L.fl_synchronize.argtypes = [vp]
        L.fl_tp_slice.argtypes = [C.POINTER(FlConfig), C.c_char_p, C.c_int32, C.c_int32, C.POINTER(C.c_int64)]
        L.fl_profile_begin.argtypes = [vp]
        L.fl_profile_end.argtypes = [vp, C.POINTER(FlKernelStat), sz, C.POINTER(sz)]
        L.fl_tune.argtypes = [C.c_char_p, C.c_int]
        L.fl_comm_probe.argtypes = [vp, C.c_int32, C.c_int64, C.c_int32, C.POINTER(C.c_double)]
        L.fl_comm_selftest.argtypes = [vp, C.c_int64, C.POINTER(C.c_int32)]
        L.fl_op_linear.argtypes = [vp, vp, vp, C.c_int64, C.c_int64, C.c_int64, C.c_int32, C.c_int32, vp, C.c_int32,
                                   C.POINTER(C.c_double)]
        L.fl_op_quantize_rows.argtypes = [vp, C.c_int32, C.c_int64, C.c_int64, vp, vp]
        L.fl_op_rmsnorm_add.argtypes = [vp, vp, C.c_int32, vp, C.c_float, C.c_int64, C.c_int64, C.c_int32, vp, vp]
        L.fl_op_norm_linear.argtypes = [C.POINTER(FlNormLinearArgs)]
        L.fl_op_linear_resid.argtypes = [C.POINTER(FlLinearResidArgs)]
        L.fl_op_gemv_resid.argtypes = [C.POINTER(FlGemvResidArgs)]
        L.fl_op_rope_kv.argtypes = [C.POINTER(FlRopeKvArgs)]
        L.fl_op_qkv_rope.argtypes = [C.POINTER(FlQkvRopeArgs)]
        L.fl_op_attn_oproj_rep.argtypes = [C.POINTER(FlAttnOprojRepArgs)]
        L.fl_op_gemv_w8.argtypes = [vp, vp, vp, vp, C.c_int64, C.c_int64, C.c_int32, vp, C.c_int32, C.POINTER(C.c_double)]
        L.fl_cache_truncate.argtypes = [vp, sz]
        L.fl_forward_verify.argtypes = [vp, vp, C.c_uint32, vp, sz, sz, vp, C.POINTER(sz), vp]
        L.fl_lookup_draft.argtypes = [vp, sz, C.POINTER(FlLookup), sz, vp, C.POINTER(sz)]
        L.fl_decode_lookup.argtypes = [vp, vp, vp, sz, C.c_uint32, sz, sz, C.c_int64, C.POINTER(FlLookup), vp, C.POINTER(sz),
                                       C.POINTER(FlSpecStats)]
        L.fl_op_verify_select.argtypes = [vp, C.c_int64, C.c_int64, vp, vp, C.POINTER(C.c_int64)]
        L.fl_forward_verify_ex.argtypes = [vp, vp, C.c_uint32, vp, sz, sz, C.POINTER(FlSampler), vp, C.POINTER(sz), vp]
        L.fl_decode_lookup_ex.argtypes = [vp, vp, vp, sz, C.c_uint32, sz, sz, C.c_int64, C.POINTER(FlLookup), C.POINTER(FlSampler), vp,
                                          C.POINTER(sz), C.POINTER(FlSpecStats)]
        L.fl_forward_verify_lp.argtypes = [vp, vp, C.c_uint32, vp, sz, sz, C.POINTER(FlSampler), C.POINTER(FlLogprobs), vp, C.POINTER(sz), vp]
        L.fl_decode_lookup_lp.argtypes = [vp, vp, vp, sz, C.c_uint32, sz, sz, C.c_int64, C.POINTER(FlLookup), C.POINTER(FlSampler),
                                          C.POINTER(FlLogprobs), vp, C.POINTER(sz), C.POINTER(FlSpecStats)]
        L.fl_op_verify_adjust.argtypes = [vp, C.c_int64, C.c_int64, vp, vp, vp, vp, C.POINTER(FlGuideDesc), vp, vp]
        L.fl_op_verify_adjust_time.argtypes = [vp, C.c_int64, C.c_int64, vp, vp, vp, vp, C.POINTER(FlGuideDesc), vp, C.c_int32, C.POINTER(C.c_double)]
        L.fl_op_rules_count.argtypes = [vp, C.c_int64, vp, C.c_int64]
        L.fl_op_verify_sample.argtypes = [vp, C.c_int64, C.c_int64, vp, C.POINTER(FlSampler), vp, C.POINTER(C.c_int64), vp]
        L.fl_op_verify_sample_time.argtypes = [vp, C.c_int64, C.c_int64, C.POINTER(FlSampler), vp, vp]
        L.fl_batch_verify.argtypes = [vp, vp, sz, vp, vp, vp, vp, vp, vp, vp]
        L.fl_batch_decode_lookup.argtypes = [vp, vp, sz, vp, vp, vp, vp, vp, vp, C.POINTER(FlLookup), vp, vp, vp, vp]
        L.fl_op_verify_packed.argtypes = [vp, C.c_int64, C.c_int64, sz, vp, vp, vp, C.c_int64, vp, vp, vp, C.c_int32, C.POINTER(C.c_double)]
        L.fl_cache_copy_prefix.argtypes = [vp, vp, sz]
        L.fl_op_kv_copy.argtypes = [vp, vp, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_int32, C.POINTER(C.c_double)]
        L.fl_encoder_create.argtypes = [C.POINTER(FlEncoderConfig), C.POINTER(FlTensor), sz, C.c_int32, C.c_int32, C.POINTER(vp)]
        L.fl_encoder_release.argtypes = [vp]
        L.fl_encoder_release.restype = None
        L.fl_encoder_hidden.argtypes = [vp, vp, sz, vp]
        L.fl_encoder_embed.argtypes = [vp, vp, vp, sz, vp]
        L.fl_op_encoder_attention.argtypes = [vp, vp, vp, vp, sz, C.c_int64, C.c_int64, C.c_int32, vp]
        L.fl_op_encoder_rows.argtypes = [C.POINTER(FlEncoderRowsArgs)]
        L.fl_op_convert_slice.argtypes = [C.POINTER(FlConvertSliceArgs)]
        L.fl_op_model_tensor.argtypes = [vp, C.c_int32, C.c_int32, C.c_int64, vp, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int32)]
        _LIB = L
    return _LIB


def _check(rc):
    if rc != 0:
        raise FastLLMError(rc, lib().fl_last_error().decode(errors="replace"))


def op_sample(logits, n_draws, temperature, seed=0, draws_done=0, top_p=None, top_k=None, return_kept=False):
    """The token-selection kernel alone on a host logits vector: n_draws successive tokens.  With top_p / top_k (fl_op_sample_ex):
    nucleus / top-k sampling; return_kept: also how many tokens each draw kept."""
    a = np.ascontiguousarray(logits, dtype=np.float32)
    out = np.zeros(n_draws, dtype=np.uint32)
    if top_p is not None or top_k is not None or return_kept:
        sp = make_sampler(temperature, seed, draws_done, top_p, top_k)
        kept = np.zeros(n_draws, dtype=np.int64)
        _check(lib().fl_op_sample_ex(a.ctypes.data, a.size, C.byref(sp), n_draws, out.ctypes.data, kept.ctypes.data))
        return (out, kept) if return_kept else out
    sp = FlSampling(temperature, seed, draws_done)
    _check(lib().fl_op_sample(a.ctypes.data, a.size, C.byref(sp), n_draws, out.ctypes.data))
    return out


def lookup_draft(history, limit, max_draft=7, ngram_max=3, ngram_min=1):
    """fl_lookup_draft (pure host): the prompt-lookup draft for `history`, at most min(max_draft, limit) ids."""
    h = np.ascontiguousarray(history, dtype=np.uint32)
    out = np.zeros(max(int(limit), 1), dtype=np.uint32)
    n = C.c_size_t(0)
    o = make_lookup(max_draft, ngram_max, ngram_min)
    _check(lib().fl_lookup_draft(h.ctypes.data if h.size else None, h.size, C.byref(o), int(limit), out.ctypes.data, C.byref(n)))
    return out[: n.value]


def op_verify_select(logits, draft):
    """The verify step's selection kernel alone: logits [T, V] float32, draft [T-1] -> (argmax uint32 [T], n_accepted)."""
    a = np.ascontiguousarray(logits, dtype=np.float32)
    T, V = a.shape
    d = np.ascontiguousarray(draft, dtype=np.uint32)
    assert d.shape == (T - 1,)
    out = np.zeros(T, dtype=np.uint32)
    n = C.c_int64(-1)
    _check(lib().fl_op_verify_select(a.ctypes.data, T, V, d.ctypes.data if d.size else None, out.ctypes.data, C.byref(n)))
    return out, n.value


def op_verify_sample(logits, draft, temperature, seed=0, draws_done=0, top_p=None, top_k=None, return_kept=False):
    """The sampled verify step's selection kernel alone: logits [T, V] float32, draft [T-1] -> (tokens uint32 [T], n_accepted); row i
    is drawn with word draws_done + i.  return_kept: also how many tokens each row's filter kept (int64 [T])."""
    a = np.ascontiguousarray(logits, dtype=np.float32)
    T, V = a.shape
    d = np.ascontiguousarray(draft, dtype=np.uint32)
    assert d.shape == (T - 1,)
    out = np.zeros(T, dtype=np.uint32)
    kept = np.zeros(T, dtype=np.int64)
    n = C.c_int64(-1)
    sp = make_sampler(temperature, seed, draws_done, top_p, top_k)
    _check(lib().fl_op_verify_sample(a.ctypes.data, T, V, d.ctypes.data if d.size else None, C.byref(sp), out.ctypes.data, C.byref(n),
                                     kept.ctypes.data if return_kept else None))
    return (out, n.value, kept) if return_kept else (out, n.value)


def _member_samplers(n, temperatures, seeds, top_p, top_k, draws_done):
    """an fl_sampler array for n members out of per-member lists (None, or a None entry: ArgMax / 0 / off), or None: ArgMax for all"""
    if temperatures is None and top_p is None and top_k is None:
        return None
    spx = (FlSampler * max(n, 1))()
    for i in range(n):
        t = temperatures[i] if temperatures is not None and temperatures[i] is not None else 0.0
        spx[i] = make_sampler(t, seeds[i] if seeds is not None and seeds[i] is not None else 0,
                              draws_done[i] if draws_done is not None and draws_done[i] is not None else 0,
                              top_p[i] if top_p is not None else None, top_k[i] if top_k is not None else None)
    return spx


def op_verify_packed(logits, members, temperatures=None, seeds=None, top_p=None, top_k=None, draws_done=None, block_rows=0, return_kept=False,
                     iters=0):
    """The packed verify step's selection kernel alone: logits [T, V] float32; members: one id list [token, *draft] per member, their
    rows back to back; per-member sampler lists as in Model.verify_packed (None: ArgMax).  The rows are cut into launches of block_rows
    rows (0: one).  Returns (tokens uint32 [T], n_accepted int64 [n]), + kept int64 [T] with return_kept, + ms per pass with iters > 0."""
    a = np.ascontiguousarray(logits, dtype=np.float32)
    T, V = a.shape
    ms_ = [np.ascontiguousarray(x, dtype=np.uint32).reshape(-1) for x in members]
    n = len(ms_)
    ids = np.ascontiguousarray(np.concatenate(ms_), dtype=np.uint32)
    offsets = np.ascontiguousarray(np.concatenate([[0], np.cumsum([x.size for x in ms_])]), dtype=np.uint64)
    assert ids.size == T
    spx = _member_samplers(n, temperatures, seeds, top_p, top_k, draws_done)
    out = np.zeros(T, dtype=np.uint32)
    acc = np.full(n, -1, dtype=np.int64)
    kept = np.zeros(T, dtype=np.int64)
    ms = C.c_double(0.0)
    _check(lib().fl_op_verify_packed(a.ctypes.data, T, V, n, offsets.ctypes.data, ids.ctypes.data, C.cast(spx, C.c_void_p) if spx is not None else None,
                                     int(block_rows), out.ctypes.data, acc.ctypes.data, kept.ctypes.data if return_kept else None, int(iters),
                                     C.byref(ms)))
    res = (out, acc) + ((kept,) if return_kept else ())
    return res + (ms.value,) if iters > 0 else res


def op_verify_sample_time(logits, temperature, iters, seed=0, top_p=None, top_k=None):
    """(ms per verify_sample launch on the T rows, ms per T one-row select_advance launches of the same rows), event-bracketed;
    iters = (repetitions of the first form, of the second), 0 skips a form."""
    a = np.ascontiguousarray(logits, dtype=np.float32)
    T, V = a.shape
    ms = (C.c_double * 2)()
    sp = make_sampler(temperature, seed, 0, top_p, top_k)
    it = (C.c_int32 * 2)(int(iters[0]), int(iters[1]))
    _check(lib().fl_op_verify_sample_time(a.ctypes.data, T, V, C.byref(sp), it, ms))
    return ms[0], ms[1]


def op_logprobs(logits, chosen, top_n):
    """The log-prob kernel alone: logits [T, V] float32, chosen [T] -> (token_logprob float32 [T], top_ids uint32 [T, top_n],
    top_logprobs float32 [T, top_n])."""
    a = np.ascontiguousarray(logits, dtype=np.float32)
    T, V = a.shape
    ch = np.ascontiguousarray(chosen, dtype=np.uint32)
    assert ch.shape == (T,)
    out = _LogprobArrays(T, top_n)
    _check(lib().fl_op_logprobs(a.ctypes.data, T, V, ch.ctypes.data, int(top_n), out.token.ctypes.data,
                                out.ids.ctypes.data if top_n > 0 else None, out.lps.ctypes.data if top_n > 0 else None))
    return out.cut(T)


def op_score(logits, targets, top_n):
    """The scoring kernel alone: logits [T, V] float32, targets [T] (SCORE_NO_TARGET: none) -> ScoreResult (logits None)."""
    a = np.ascontiguousarray(logits, dtype=np.float32)
    T, V = a.shape
    out = _ScoreArrays(T, top_n, targets)
    _check(lib().fl_op_score(a.ctypes.data, T, V, out.targets.ctypes.data, int(top_n), out.lp.ctypes.data, out.rank.ctypes.data,
                             out.ids.ctypes.data if top_n > 0 else None, out.lps.ctypes.data if top_n > 0 else None))
    return out.result()


def op_score_time(logits, targets, top_n, iters):
    """ms per score_rows launch on the T rows: the mean of `iters` back-to-back launches between two events."""
    a = np.ascontiguousarray(logits, dtype=np.float32)
    T, V = a.shape
    tg = np.ascontiguousarray(targets, dtype=np.uint32)
    assert tg.shape == (T,)
    ms = C.c_double(0.0)
    _check(lib().fl_op_score_time(a.ctypes.data, T, V, tg.ctypes.data, int(top_n), int(iters), C.byref(ms)))
    return ms.value


def op_logit_rules(logits, words, biases, scalars, tokens, count_input=True, has_rules=None):
    """The logit-rules kernel alone (batch form): logits float32 [B, V], words uint32 [B, V], biases float32 [B, V], scalars [B, 3]
    (repetition, frequency, presence penalty), tokens [B] (an id >= V: none) -> (adjusted rows float32 [B, V], words after the
    launch uint32 [B, V]).  has_rules [B]: a false entry makes the row's table entry null (the row is copied through)."""
    a = np.ascontiguousarray(logits, dtype=np.float32)
    B, V = a.shape
    w = np.array(words, dtype=np.uint32, order="C").reshape(B, V)
    bs = np.ascontiguousarray(biases, dtype=np.float32).reshape(B, V)
    sc = np.ascontiguousarray(scalars, dtype=np.float32).reshape(B, 3)
    tk = np.ascontiguousarray(tokens, dtype=np.uint32).reshape(B)
    hr = None if has_rules is None else np.ascontiguousarray(has_rules, dtype=np.uint8).reshape(B)
    out = np.empty((B, V), dtype=np.float32)
    _check(lib().fl_op_logit_rules(a.ctypes.data, B, V, w.ctypes.data, bs.ctypes.data, sc.ctypes.data, tk.ctypes.data, 1 if count_input else 0,
                                   hr.ctypes.data if hr is not None else None, out.ctypes.data))
    return out, w


def op_guide_mask(logits, row_ptr, tokens, next, states, input_tokens, has_guide=None):
    """The guided-decoding kernel alone (batch form): logits float32 [B, V], one automaton (CSR row_ptr / tokens / next), states [B]
    and input_tokens [B] (row b first moves from states[b] along input_tokens[b]; no such edge, or an id >= V: it stays)
    -> (masked rows float32 [B, V], the states the rows were masked in uint32 [B]).  has_guide [B]: a false entry makes the row's
    control block null (the row is copied through)."""
    a = np.ascontiguousarray(logits, dtype=np.float32)
    B, V = a.shape
    st, keep = make_guide_desc(row_ptr, tokens, next)
    ss = np.ascontiguousarray(states, dtype=np.uint32).reshape(B)
    tk = np.ascontiguousarray(input_tokens, dtype=np.uint32).reshape(B)
    hg = None if has_guide is None else np.ascontiguousarray(has_guide, dtype=np.uint8).reshape(B)
    out = np.empty((B, V), dtype=np.float32)
    nxt = np.zeros(B, dtype=np.uint32)
    _check(lib().fl_op_guide_mask(a.ctypes.data, B, V, C.byref(st), ss.ctypes.data, tk.ctypes.data, hg.ctypes.data if hg is not None else None,
                                  out.ctypes.data, nxt.ctypes.data))
    del keep
    return out, nxt


def _verify_adjust_call(logits, ids, words, biases, scalars, guide, states):
    """The arguments op_verify_adjust and its timed form share: (pointer list up to `states`, T, V, the words array or None, what must stay alive)."""
    a = np.ascontiguousarray(logits, dtype=np.float32)
    T, V = a.shape
    tk = np.ascontiguousarray(ids, dtype=np.uint32).reshape(T)
    w = bs = sc = None
    if words is not None:
        w = np.array(words, dtype=np.uint32, order="C").reshape(V)
        bs = np.ascontiguousarray(biases, dtype=np.float32).reshape(V)
        sc = np.ascontiguousarray(scalars, dtype=np.float32).reshape(3)
    st = keep = ss = None
    if guide is not None:
        st, keep = make_guide_desc(*guide)
        ss = np.ascontiguousarray(states, dtype=np.uint32).reshape(T)
    ptr = lambda x: x.ctypes.data if x is not None else None
    args = [a.ctypes.data, T, V, tk.ctypes.data, ptr(w), ptr(bs), ptr(sc), C.byref(st) if st is not None else None, ptr(ss)]
    return args, T, V, w, (a, tk, bs, sc, st, keep, ss)


def op_verify_adjust(logits, ids, words=None, biases=None, scalars=None, guide=None, states=None):
    """verify_adjust_kernel alone: logits float32 [T, V] (the rows of one verify step, T <= 16) and ids [T] (row i's input id).  Rules:
    words uint32 [V], biases float32 [V], scalars (repetition, frequency, presence penalty); guide: (row_ptr, tokens, next) with states
    [T], the state each row is masked in.  At least one of the two.  Returns (adjusted rows float32 [T, V], words after the launches --
    the table is only read, so they must be the words that went in -- or None without rules)."""
    args, T, V, w, keep = _verify_adjust_call(logits, ids, words, biases, scalars, guide, states)
    out = np.empty((T, V), dtype=np.float32)
    _check(lib().fl_op_verify_adjust(*args, out.ctypes.data))
    del keep
    return out, w


def op_verify_adjust_time(logits, ids, iters, words=None, biases=None, scalars=None, guide=None, states=None):
    """op_verify_adjust timed: ms per launch, the mean of `iters` back-to-back launches between two events."""
    args, _, _, _, keep = _verify_adjust_call(logits, ids, words, biases, scalars, guide, states)
    ms = C.c_double(0.0)
    _check(lib().fl_op_verify_adjust_time(*args, int(iters), C.byref(ms)))
    del keep
    return ms.value


def op_rules_count(words, ids):
    """rules_count_kernel alone: ids (at most 16) counted into words uint32 [V], in order -> the words after the launch."""
    w = np.array(words, dtype=np.uint32, order="C").reshape(-1)
    tk = np.ascontiguousarray(ids, dtype=np.uint32).reshape(-1)
    _check(lib().fl_op_rules_count(w.ctypes.data, w.size, tk.ctypes.data if tk.size else None, tk.size))
    return w


def abi_version():
    return lib().fl_abi_version()


def device_count():
    n = C.c_int(0)
    _check(lib().fl_device_count(C.byref(n)))
    return n.value


def comm_unique_id():
    buf = C.create_string_buffer(UNIQUE_ID_BYTES)
    _check(lib().fl_comm_unique_id(buf))
    return buf.raw


def make_config(cfg):
    c = FlConfig()
    c.family = FAMILY[cfg["family"]] if isinstance(cfg["family"], str) else int(cfg["family"])
    c.qkv_bias = int(cfg.get("qkv_bias", cfg["family"] == "qwen2"))
    c.hidden_size = cfg["hidden_size"]
    c.intermediate_size = cfg["intermediate_size"]
    c.vocab_size = cfg["vocab_size"]
    c.num_hidden_layers = cfg["num_hidden_layers"]
    c.num_attention_heads = cfg["num_attention_heads"]
    c.num_key_value_heads = cfg.get("num_key_value_heads") or 0
    c.max_position_embeddings = cfg.get("max_position_embeddings") or 0
    c.sliding_window = cfg.get("sliding_window") or 0
    c.rms_norm_eps = cfg["rms_norm_eps"]
    c.rope_theta = cfg.get("rope_theta") or 0.0
    return c


def tp_slice(cfg, name, rank, tp):
    out = (C.c_int64 * 4)()
    c = make_config(cfg)
    _check(lib().fl_tp_slice(C.byref(c), name.encode(), rank, tp, out))
    return tuple(out)


def _np_dtype_code(a):
    if a.dtype == np.float32:
        return F32
    if a.dtype == np.uint16:
        return BF16
    if a.dtype == np.float16:
        return F16
    raise TypeError("unsupported array dtype %s" % a.dtype)


def _tensor_array(tensors):
    """dict name -> numpy array | (device_ptr, dtype_code, shape, device_ordinal)  ->  (FlTensor array, objects to keep alive)"""
    arr = (FlTensor * len(tensors))()
    keep = []
    for i, (name, a) in enumerate(tensors.items()):
        arr[i].name = name.encode()
        if isinstance(a, tuple):
            ptr, code, shape, dev = a
            arr[i].dtype, arr[i].ndim, arr[i].data, arr[i].device = code, len(shape), ptr, dev
            for j, s in enumerate(shape):
                arr[i].shape[j] = s
        else:
            a = np.ascontiguousarray(a)
            keep.append(a)
            arr[i].dtype, arr[i].ndim, arr[i].data, arr[i].device = _np_dtype_code(a), a.ndim, a.ctypes.data, -1
            for j, s in enumerate(a.shape):
                arr[i].shape[j] = s
    return arr, keep


class Encoder:
    """fl_encoder handle: the BERT / MiniLM encoder forward (embeddings).  cfg: dict with hidden_size, intermediate_size,
    num_hidden_layers, num_attention_heads, max_position_embeddings, vocab_size, layer_norm_eps; tensors as for Model (HF names
    without the "bert." prefix)."""

    def __init__(self, cfg, tensors, dtype="bf16", activation="gelu_tanh", add_token_type0=False, max_batch_tokens=0, device=0):
        self.cfg = dict(cfg)
        self.h = cfg["hidden_size"]
        arr, keep = _tensor_array(tensors)
        c = make_encoder_config(cfg, activation, add_token_type0, max_batch_tokens)
        h = C.c_void_p()
        _check(lib().fl_encoder_create(C.byref(c), arr, len(tensors), BF16 if dtype == "bf16" else F32, device, C.byref(h)))
        del keep
        self._h = h

    def hidden(self, ids):
        """fl_encoder_hidden: last hidden states [T, h] float32 of one sequence."""
        ids = np.ascontiguousarray(ids, dtype=np.uint32)
        out = np.empty((ids.size, self.h), dtype=np.float32)
        _check(lib().fl_encoder_hidden(self._h, ids.ctypes.data, ids.size, out.ctypes.data))
        return out

    def embed(self, seqs):
        """fl_encoder_embed: seqs is a list of id lists; returns [len(seqs), h] float32 (mean-pooled, L2-normalised)."""
        seqs = [np.asarray(s, dtype=np.uint32).reshape(-1) for s in seqs]
        offs = np.zeros(len(seqs) + 1, dtype=np.uint64)
        offs[1:] = np.cumsum([s.size for s in seqs])
        ids = np.concatenate(seqs) if seqs else np.zeros(0, np.uint32)
        out = np.empty((len(seqs), self.h), dtype=np.float32)
        _check(lib().fl_encoder_embed(self._h, ids.ctypes.data if ids.size else None, offs.ctypes.data, len(seqs), out.ctypes.data))
        return out

    def close(self):
        if getattr(self, "_h", None):
            lib().fl_encoder_release(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def op_encoder_attention(q, k, v, lengths, H, d):
    """The encoder's unmasked ragged attention kernel alone.  q / k / v [sum(lengths), H*d], all uint16 (bf16 bits: the MFMA kernel)
    or all float32 (the VALU kernel); returns [sum(lengths), H*d] float32."""
    q, k, v = (np.ascontiguousarray(a) for a in (q, k, v))
    assert q.dtype == k.dtype == v.dtype and q.shape == k.shape == v.shape == (int(sum(lengths)), H * d)
    offs = np.zeros(len(lengths) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum(lengths)
    out = np.empty(q.shape, dtype=np.float32)
    _check(lib().fl_op_encoder_attention(q.ctypes.data, k.ctypes.data, v.ctypes.data, offs.ctypes.data, len(lengths), H, d,
                                         _np_dtype_code(q), out.ctypes.data))
    return out


def _encoder_rows(form, dtype, T, h, out_rows, keep, repeat=1, **fields):
    """one fl_op_encoder_rows call; fields: name -> array (its pointer), int or float.  Returns (x_res_out [T, h] float32 for forms 0
    and 1, out [out_rows, h] as stored: uint16 bf16 bits or float32)."""
    bf16 = dtype == "bf16"
    a = FlEncoderRowsArgs()
    a.struct_size = C.sizeof(FlEncoderRowsArgs)
    a.form, a.dtype, a.repeat, a.n_slab, a.T, a.h = form, BF16 if bf16 else F32, repeat, 1, T, h
    for name, v in fields.items():
        setattr(a, name, v.ctypes.data if isinstance(v, np.ndarray) else v)
    x_res = np.empty((T, h), np.float32) if form <= 1 else None
    out = np.empty((out_rows, h), np.uint16 if bf16 and form != 3 else np.float32)
    a.x_res_out, a.out = _ptr(x_res), out.ctypes.data
    _check(lib().fl_op_encoder_rows(C.byref(a)))
    del keep
    return x_res, out


def _offsets(lengths):
    offs = np.zeros(len(lengths) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum(lengths)
    return offs


def op_encoder_embed_ln(word, pos, ids, lengths, ln_w, ln_b, eps, dtype, tt0=None, repeat=1):
    """launch_encoder_embed_ln alone (fl_op_encoder_rows form 0): word [vocab, h], pos [P, h] and tt0 [h] (optional) as uint16 bf16 bits
    (dtype "bf16") or float32; ids [sum(lengths)]; sequence s owns lengths[s] rows.  Returns (x_res [T, h] float32, xn [T, h] as
    stored)."""
    et = np.uint16 if dtype == "bf16" else np.float32
    word, pos = np.ascontiguousarray(word, dtype=et), np.ascontiguousarray(pos, dtype=et)
    tt0 = np.ascontiguousarray(tt0, dtype=et) if tt0 is not None else None
    ids, offs, ln_w, ln_b = np.ascontiguousarray(ids, dtype=np.uint32), _offsets(lengths), _f32(ln_w), _f32(ln_b)
    T, h = int(offs[-1]), word.shape[1]
    assert ids.shape == (T,) and pos.shape[1] == h and ln_w.shape == ln_b.shape == (h,) and (tt0 is None or tt0.shape == (h,))
    return _encoder_rows(0, dtype, T, h, T, (word, pos, tt0, ids, offs, ln_w, ln_b), repeat, word=word, pos=pos, tt0=_ptr(tt0), ids=ids,
                         offsets=offs, n_seq=len(lengths), vocab=word.shape[0], P=pos.shape[0], ln_w=ln_w, ln_b=ln_b, eps=eps)


def op_encoder_add_ln(x, slabs, ln_w, ln_b, eps, dtype, bias=None, repeat=1):
    """launch_encoder_add_ln alone (fl_op_encoder_rows form 1): x [T, h] and slabs [n_slab, T, h] float32, bias [h] (optional).
    Returns (x_res [T, h] float32 after the call, xn [T, h] as stored: uint16 bf16 bits or float32)."""
    x, slabs, ln_w, ln_b = _f32(x), _f32(slabs), _f32(ln_w), _f32(ln_b)
    bias = _f32(bias) if bias is not None else None
    T, h = x.shape
    assert slabs.shape[1:] == (T, h) and ln_w.shape == ln_b.shape == (h,) and (bias is None or bias.shape == (h,))
    return _encoder_rows(1, dtype, T, h, T, (x, slabs, ln_w, ln_b, bias), repeat, x=x, slabs=slabs, n_slab=slabs.shape[0], bias=_ptr(bias),
                         ln_w=ln_w, ln_b=ln_b, eps=eps)


def op_encoder_bias_act(slabs, dtype, bias=None, act=None, repeat=1):
    """launch_encoder_bias_act alone (fl_op_encoder_rows form 2): slabs [n_slab, T, N] float32, bias [N] (optional), act None /
    "gelu_tanh" / "gelu_erf" (ENC_ACT).  Returns out [T, N] as stored: uint16 bf16 bits or float32."""
    slabs = _f32(slabs)
    bias = _f32(bias) if bias is not None else None
    n_slab, T, N = slabs.shape
    assert bias is None or bias.shape == (N,)
    return _encoder_rows(2, dtype, T, N, T, (slabs, bias), repeat, slabs=slabs, n_slab=n_slab, bias=_ptr(bias),
                         act=act if isinstance(act, int) else ENC_ACT[act])[1]


def op_encoder_pool_l2(x, lengths, repeat=1):
    """launch_encoder_pool_l2 alone (fl_op_encoder_rows form 3): x [sum(lengths), h] float32; returns the L2-normalised mean of each
    member's rows, [len(lengths), h] float32."""
    x, offs = _f32(x), _offsets(lengths)
    T, h = x.shape
    assert T == int(offs[-1])
    return _encoder_rows(3, "f32", T, h, len(lengths), (x, offs), repeat, x=x, offsets=offs, n_seq=len(lengths))[1]


def op_convert_slice(src, r0, c0, rows, cols, dst_dtype, dst_rows, dst_ld, dst_row0=0, row_mode=0, head_pad=0, dm=0, d=0, via_bf16=False):
    """launch_convert_slice alone (fl_op_convert_slice): src [R, C] float32 / float16 / uint16 bf16 bits; dst_dtype "bf16" or "f32"
    (via_bf16: the fp32 of the value rounded to bf16).
    Returns the whole destination [dst_rows, dst_ld] as bit patterns (uint16 / uint32); what the launch left alone is all ones."""
    src = np.ascontiguousarray(src)
    assert src.ndim == 2
    out = np.zeros((max(int(dst_rows), 1), max(int(dst_ld), 1)), np.uint16 if dst_dtype == "bf16" else np.uint32)
    a = FlConvertSliceArgs()
    a.struct_size = C.sizeof(FlConvertSliceArgs)
    a.src_dtype, a.dst_dtype, a.row_mode, a.head_pad = _np_dtype_code(src), BF16 if dst_dtype == "bf16" else F32, row_mode, head_pad
    a.R, a.C, a.r0, a.c0, a.rows, a.cols = src.shape[0], src.shape[1], r0, c0, rows, cols
    a.dst_rows, a.dst_ld, a.dst_row0, a.dm, a.d, a.via_bf16 = dst_rows, dst_ld, dst_row0, dm, d, int(via_bf16)
    a.src, a.dst = src.ctypes.data, out.ctypes.data
    _check(lib().fl_op_convert_slice(C.byref(a)))
    return out


class Model:
    """fl_model handle.  tensors: dict name -> numpy array (float32 / float16 / uint16 bf16 bits), or
    name -> (device_ptr, dtype_code, shape, device_ordinal) for tensors already in HBM.
    decode_weights: None / "compute" (fl_model_create) or "e4m3" (FL_WEIGHTS_E4M3_ROW: the decode step streams FP8 weights; an int
    is passed through as the fl_weight_format value)."""

    def __init__(self, cfg, tensors, dtype="bf16", tp_mode=TP_NONE, tp_size=1, tp_rank=0, device_ids=None,
                 unique_id=None, decode_weights=None):
        L = lib()
        self.cfg = dict(cfg)
        self.V = cfg["vocab_size"]
        arr = (FlTensor * len(tensors))()
        keep = []
        for i, (name, a) in enumerate(tensors.items()):
            arr[i].name = name.encode()
            if isinstance(a, tuple):
                ptr, code, shape, dev = a
                arr[i].dtype, arr[i].ndim, arr[i].data, arr[i].device = code, len(shape), ptr, dev
                for j, s in enumerate(shape):
                    arr[i].shape[j] = s
            else:
                a = np.ascontiguousarray(a)
                keep.append(a)
                arr[i].dtype, arr[i].ndim, arr[i].data, arr[i].device = _np_dtype_code(a), a.ndim, a.ctypes.data, -1
                for j, s in enumerate(a.shape):
                    arr[i].shape[j] = s
        par = FlParallel()
        par.mode, par.tp_size, par.tp_rank = tp_mode, tp_size, tp_rank
        if device_ids is not None:
            ids = (C.c_int32 * len(device_ids))(*device_ids)
            par.device_ids, par.n_device_ids = ids, len(device_ids)
        uid = None
        if unique_id is not None:
            uid = C.create_string_buffer(bytes(unique_id), UNIQUE_ID_BYTES)
            par.unique_id = C.cast(uid, C.c_void_p)
        c = make_config(cfg)
        h = C.c_void_p()
        code = BF16 if dtype == "bf16" else F32
        if decode_weights is None:
            _check(L.fl_model_create(C.byref(c), arr, len(tensors), code, C.byref(par), C.byref(h)))
        else:
            opts = FlModelOptions()
            opts.struct_size = C.sizeof(FlModelOptions)
            opts.decode_weights = decode_weights if isinstance(decode_weights, int) else DECODE_WEIGHTS[decode_weights]
            _check(L.fl_model_create_opts(C.byref(c), arr, len(tensors), code, C.byref(par), C.byref(opts), C.byref(h)))
        self._h = h

    def info(self):
        out = FlModelInfo()
        _check(lib().fl_model_get_info(self._h, C.byref(out)))
        return out

    def new_cache(self, max_seq):
        return Cache(self, max_seq)

    def tensor(self, name, layer=0, shard=0, shape_only=False):
        """fl_op_model_tensor: the device tensor `name` (MODEL_TENSORS) of a local shard as it lies in HBM -- bit patterns: uint16 for
        bf16, uint32 for fp32 weights; float32 for norms, biases, scales and the RoPE tables; uint8 for e4m3 bytes.  shape_only: (rows,
        cols, element code) without a copy."""
        r, c, e = C.c_int64(0), C.c_int64(0), C.c_int32(-1)
        sel = name if isinstance(name, int) else MODEL_TENSORS[name]
        _check(lib().fl_op_model_tensor(self._h, shard, sel, layer, None, C.byref(r), C.byref(c), C.byref(e)))
        if shape_only:
            return r.value, c.value, e.value
        plain_f32 = sel in (1, 3, 4, 6, 10, 11) or (sel >= 12 and sel % 2 == 1)
        dt = np.uint8 if e.value == ELEM_E4M3 else np.uint16 if e.value == BF16 else np.float32 if plain_f32 else np.uint32
        out = np.empty((r.value, c.value), dt)
        _check(lib().fl_op_model_tensor(self._h, shard, sel, layer, out.ctypes.data, C.byref(r), C.byref(c), C.byref(e)))
        return out

    def forward(self, cache, ids, pos):
        ids = np.ascontiguousarray(ids, dtype=np.uint32)
        out = np.empty(self.V, dtype=np.float32)
        _check(lib().fl_forward(self._h, cache._h, ids.ctypes.data, ids.size, pos, out.ctypes.data))
        return out

    def forward_argmax(self, cache, ids, pos):
        ids = np.ascontiguousarray(ids, dtype=np.uint32)
        tok = C.c_uint32(0)
        _check(lib().fl_forward_argmax(self._h, cache._h, ids.ctypes.data, ids.size, pos, C.byref(tok)))
        return tok.value

    def decode_greedy(self, cache, first_token, pos, n_steps, eos=-1):
        toks = np.zeros(max(n_steps, 1), dtype=np.uint32)
        n = C.c_size_t(0)
        _check(lib().fl_decode_greedy(self._h, cache._h, int(first_token), pos, n_steps, eos, toks.ctypes.data, C.byref(n)))
        return toks[: n.value]

    def forward_verify(self, cache, token, draft, pos, want_logits=False, temperature=None, top_p=None, top_k=None, seed=0, draws_done=0):
        """fl_forward_verify: one forward of [token, *draft]; returns (tokens, logits [len(draft) + 1, V] or None) -- the accepted
        drafts followed by the model's own next token.  With a temperature (fl_forward_verify_ex): row i is DRAWN with word
        draws_done + i of the seeded stream; the request has consumed len(tokens) words afterwards."""
        d = np.ascontiguousarray(draft, dtype=np.uint32)
        toks = np.zeros(d.size + 1, dtype=np.uint32)
        lg = np.empty((d.size + 1, self.V), dtype=np.float32) if want_logits else None
        n = C.c_size_t(0)
        if temperature is not None:
            sp = make_sampler(temperature, seed, draws_done, top_p, top_k)
            _check(lib().fl_forward_verify_ex(self._h, cache._h, int(token), d.ctypes.data if d.size else None, d.size, pos, C.byref(sp),
                                              toks.ctypes.data, C.byref(n), lg.ctypes.data if want_logits else None))
            return toks[: n.value], lg
        _check(lib().fl_forward_verify(self._h, cache._h, int(token), d.ctypes.data if d.size else None, d.size, pos, toks.ctypes.data,
                                       C.byref(n), lg.ctypes.data if want_logits else None))
        return toks[: n.value], lg

    def decode_lookup(self, cache, corpus, first_token, pos, n_steps, eos=-1, max_draft=7, ngram_max=3, ngram_min=1, return_stats=False,
                      temperature=None, top_p=None, top_k=None, seed=0, draws_done=0):
        """fl_decode_lookup: the greedy loop built from verify steps with prompt-lookup drafts out of corpus ++ [first_token] ++ output.
        return_stats: also a dict(steps, drafted, accepted).  With a temperature (fl_decode_lookup_ex): the loop of decode_sample, token
        k drawn with word draws_done + k."""
        cp = np.ascontiguousarray(corpus, dtype=np.uint32)
        toks = np.zeros(max(n_steps, 1), dtype=np.uint32)
        n = C.c_size_t(0)
        o = make_lookup(max_draft, ngram_max, ngram_min)
        st = FlSpecStats()
        if temperature is not None:
            sp = make_sampler(temperature, seed, draws_done, top_p, top_k)
            _check(lib().fl_decode_lookup_ex(self._h, cache._h, cp.ctypes.data if cp.size else None, cp.size, int(first_token), pos, n_steps,
                                             eos, C.byref(o), C.byref(sp), toks.ctypes.data, C.byref(n), C.byref(st)))
        else:
            _check(lib().fl_decode_lookup(self._h, cache._h, cp.ctypes.data if cp.size else None, cp.size, int(first_token), pos, n_steps, eos,
                                          C.byref(o), toks.ctypes.data, C.byref(n), C.byref(st)))
        if return_stats:
            return toks[: n.value], dict(steps=st.steps, drafted=st.drafted, accepted=st.accepted)
        return toks[: n.value]

    def forward_verify_lp(self, cache, token, draft, pos, logprobs=None, temperature=None, top_p=None, top_k=None, seed=0, draws_done=0,
                          want_logits=False):
        """fl_forward_verify_lp: forward_verify on a cache that may have logit rules and / or a guide.  Returns (tokens, logits): the
        accepted drafts followed by the model's own next token, and the RAW rows [len(draft) + 1, V] (None without want_logits; with a
        guide only the rows of the draft the guide can reach are written).  logprobs = N: (tokens, logits, token_logprob [n], top_ids
        [n, N], top_logprobs [n, N]) -- the model's own distribution for every returned token."""
        d = np.ascontiguousarray(draft, dtype=np.uint32)
        toks = np.zeros(d.size + 1, dtype=np.uint32)
        lg = np.empty((d.size + 1, self.V), dtype=np.float32) if want_logits else None
        n = C.c_size_t(0)
        sp = make_sampler(temperature, seed, draws_done, top_p, top_k) if temperature is not None else None
        lp = _LogprobArrays(d.size + 1, logprobs) if logprobs is not None else None
        st = lp.struct() if lp is not None else None
        _check(lib().fl_forward_verify_lp(self._h, cache._h, int(token), d.ctypes.data if d.size else None, d.size, pos,
                                          C.byref(sp) if sp is not None else None, C.byref(st) if st is not None else None, toks.ctypes.data,
                                          C.byref(n), lg.ctypes.data if want_logits else None))
        res = (toks[: n.value], lg)
        return res + lp.cut(n.value) if lp is not None else res

    def decode_lookup_lp(self, cache, corpus, first_token, pos, n_steps, eos=-1, max_draft=7, ngram_max=3, ngram_min=1, return_stats=False,
                         logprobs=None, temperature=None, top_p=None, top_k=None, seed=0, draws_done=0):
        """fl_decode_lookup_lp: decode_lookup on a cache that may have logit rules and / or a guide -- the loop of decode_sample with the
        same rules, guide and sampler.  Returns the tokens; with logprobs = N: (tokens, token_logprob [n], top_ids [n, N], top_logprobs
        [n, N]); return_stats appends a dict(steps, drafted, accepted)."""
        cp = np.ascontiguousarray(corpus, dtype=np.uint32)
        toks = np.zeros(max(n_steps, 1), dtype=np.uint32)
        n = C.c_size_t(0)
        o = make_lookup(max_draft, ngram_max, ngram_min)
        stats = FlSpecStats()
        sp = make_sampler(temperature, seed, draws_done, top_p, top_k) if temperature is not None else None
        lp = _LogprobArrays(n_steps, logprobs) if logprobs is not None else None
        st = lp.struct() if lp is not None else None
        _check(lib().fl_decode_lookup_lp(self._h, cache._h, cp.ctypes.data if cp.size else None, cp.size, int(first_token), pos, n_steps, eos,
                                         C.byref(o), C.byref(sp) if sp is not None else None, C.byref(st) if st is not None else None,
                                         toks.ctypes.data, C.byref(n), C.byref(stats)))
        res = (toks[: n.value],)
        if lp is not None:
            res += lp.cut(n.value)
        if return_stats:
            res += (dict(steps=stats.steps, drafted=stats.drafted, accepted=stats.accepted),)
        return res[0] if len(res) == 1 else res

    def verify_packed(self, caches, tokens, drafts, pos, temperatures=None, seeds=None, top_p=None, top_k=None, draws_done=None, want_logits=False):
        """fl_batch_verify: the verify steps [tokens[i], *drafts[i]] of caches[i] at RoPE offset pos[i], all in ONE forward.  Per member
        the result of forward_verify(caches[i], tokens[i], drafts[i], pos[i], ..): temperatures / seeds / top_p / top_k / draws_done are
        lists (None, or a None entry: ArgMax / 0 / off / 0).  Returns a list of per-member id arrays -- the accepted drafts followed by
        the model's own next token -- or (that list, logits [total rows, V] in pack order) with want_logits."""
        n = len(caches)
        assert len(tokens) == n and len(drafts) == n
        ms = [np.concatenate([[int(tokens[i])], np.asarray(drafts[i], dtype=np.uint32).reshape(-1)]).astype(np.uint32) for i in range(n)]
        ids = np.ascontiguousarray(np.concatenate(ms) if ms else np.zeros(0, np.uint32), dtype=np.uint32)
        offsets = np.ascontiguousarray(np.concatenate([[0], np.cumsum([x.size for x in ms])]), dtype=np.uint64)
        pos = np.ascontiguousarray(pos, dtype=np.uint64)
        assert pos.shape == (n,)
        arr = (C.c_void_p * max(n, 1))(*[c._h for c in caches])
        spx = _member_samplers(n, temperatures, seeds, top_p, top_k, draws_done)
        toks = np.zeros(max(ids.size, 1), dtype=np.uint32)
        cnt = np.zeros(max(n, 1), dtype=np.uint64)
        lg = np.empty((ids.size, self.V), dtype=np.float32) if want_logits else None
        _check(lib().fl_batch_verify(self._h, C.cast(arr, C.c_void_p), n, ids.ctypes.data, offsets.ctypes.data, pos.ctypes.data,
                                     C.cast(spx, C.c_void_p) if spx is not None else None, toks.ctypes.data, cnt.ctypes.data,
                                     lg.ctypes.data if want_logits else None))
        got = [toks[int(offsets[i]): int(offsets[i]) + int(cnt[i])].copy() for i in range(n)]
        return (got, lg) if want_logits else got

    def decode_lookup_packed(self, caches, corpora, first_tokens, pos, n_steps, eos=None, max_draft=7, ngram_max=3, ngram_min=1,
                             temperatures=None, seeds=None, top_p=None, top_k=None, draws_done=None, return_stats=False):
        """fl_batch_decode_lookup: decode_lookup for every member, each iteration ONE packed verify step over the unfinished members.
        corpora / first_tokens / pos / n_steps: one entry per member; eos: a list (None or a negative entry: none).  Returns a list of
        per-member id arrays, or (that list, [dict(steps, drafted, accepted)] per member) with return_stats."""
        n = len(caches)
        cps = [np.ascontiguousarray(x, dtype=np.uint32).reshape(-1) for x in corpora]
        assert len(cps) == n and len(first_tokens) == n and len(pos) == n and len(n_steps) == n
        corpus = np.ascontiguousarray(np.concatenate(cps) if cps else np.zeros(0, np.uint32), dtype=np.uint32)
        coff = np.ascontiguousarray(np.concatenate([[0], np.cumsum([x.size for x in cps])]), dtype=np.uint64)
        first = np.ascontiguousarray(first_tokens, dtype=np.uint32)
        pos = np.ascontiguousarray(pos, dtype=np.uint64)
        steps = np.ascontiguousarray(n_steps, dtype=np.uint64)
        eos_a = None if eos is None else np.ascontiguousarray([-1 if e is None else e for e in eos], dtype=np.int64)
        stride = int(steps.max()) if n else 0
        arr = (C.c_void_p * max(n, 1))(*[c._h for c in caches])
        spx = _member_samplers(n, temperatures, seeds, top_p, top_k, draws_done)
        o = make_lookup(max_draft, ngram_max, ngram_min)
        toks = np.zeros((max(n, 1), max(stride, 1)), dtype=np.uint32)
        cnt = np.zeros(max(n, 1), dtype=np.uint64)
        st = (FlSpecStats * max(n, 1))()
        _check(lib().fl_batch_decode_lookup(self._h, C.cast(arr, C.c_void_p), n, corpus.ctypes.data if corpus.size else None, coff.ctypes.data,
                                            first.ctypes.data, pos.ctypes.data, steps.ctypes.data, eos_a.ctypes.data if eos_a is not None else None,
                                            C.byref(o), C.cast(spx, C.c_void_p) if spx is not None else None, toks.ctypes.data, cnt.ctypes.data,
                                            C.cast(st, C.c_void_p)))
        got = [toks[i, : int(cnt[i])].copy() for i in range(n)]
        if return_stats:
            return got, [dict(steps=st[i].steps, drafted=st[i].drafted, accepted=st[i].accepted) for i in range(n)]
        return got

    def forward_sample(self, cache, ids, pos, temperature, seed=0, draws_done=0, top_p=None, top_k=None, logprobs=None):
        """logprobs = N (0: the chosen token's only): returns (token, token_logprob [1], top_ids [1, N], top_logprobs [1, N]) --
        log-softmax of the model's own logits (temperature 1, nothing masked), computed on the device."""
        ids = np.ascontiguousarray(ids, dtype=np.uint32)
        tok = C.c_uint32(0)
        if logprobs is not None:
            sp = make_sampler(temperature, seed, draws_done, top_p, top_k)
            lp = _LogprobArrays(1, logprobs)
            st = lp.struct()
            _check(lib().fl_forward_sample_lp(self._h, cache._h, ids.ctypes.data, ids.size, pos, C.byref(sp), C.byref(tok), C.byref(st)))
            return (tok.value,) + lp.cut(1)
        if top_p is not None or top_k is not None:
            sp = make_sampler(temperature, seed, draws_done, top_p, top_k)
            _check(lib().fl_forward_sample_ex(self._h, cache._h, ids.ctypes.data, ids.size, pos, C.byref(sp), C.byref(tok)))
            return tok.value
        sp = FlSampling(temperature, seed, draws_done)
        _check(lib().fl_forward_sample(self._h, cache._h, ids.ctypes.data, ids.size, pos, C.byref(sp), C.byref(tok)))
        return tok.value

    def prefill_packed(self, caches, prompts, pos=None, temperatures=None, seeds=None, top_p=None, top_k=None, want_logits=False):
        """fl_batch_prefill: prompts[i] appended to caches[i] at RoPE offset pos[i] (None: 0 for all), all in ONE forward.  Per member
        the result of forward_sample(caches[i], prompts[i], pos[i], ..): temperatures / seeds / top_p / top_k are lists (None, or a None
        entry: ArgMax / 0 / off).  Returns the tokens [n], or (tokens, logits [n, V]) with want_logits."""
        n = len(caches)
        assert len(prompts) == n
        ps = [np.ascontiguousarray(p, dtype=np.uint32).reshape(-1) for p in prompts]
        ids = np.ascontiguousarray(np.concatenate(ps) if ps else np.zeros(0, np.uint32), dtype=np.uint32)
        offsets = np.ascontiguousarray(np.concatenate([[0], np.cumsum([p.size for p in ps])]), dtype=np.uint64)
        pos = np.ascontiguousarray([0] * n if pos is None else pos, dtype=np.uint64)
        arr = (C.c_void_p * max(n, 1))(*[c._h for c in caches])
        spx = None
        if temperatures is not None or top_p is not None or top_k is not None:
            spx = (FlSampler * max(n, 1))()
            for i in range(n):
                t = temperatures[i] if temperatures is not None and temperatures[i] is not None else 0.0
                spx[i] = make_sampler(t, seeds[i] if seeds is not None and seeds[i] is not None else 0, 0,
                                      top_p[i] if top_p is not None else None, top_k[i] if top_k is not None else None)
        toks = np.zeros(max(n, 1), dtype=np.uint32)
        lg = np.empty((n, self.V), dtype=np.float32) if want_logits else None
        _check(lib().fl_batch_prefill(self._h, C.cast(arr, C.c_void_p), n, ids.ctypes.data, offsets.ctypes.data, pos.ctypes.data,
                                      C.cast(spx, C.c_void_p) if spx is not None else None, toks.ctypes.data,
                                      lg.ctypes.data if want_logits else None))
        return (toks[:n], lg) if want_logits else toks[:n]

    def embed_packed(self, caches, seqs, pos=None, pooling="last", mask="causal", normalize=True, dimensions=0):
        """fl_batch_embed: seqs[i] appended to caches[i] at RoPE offset pos[i] (None: 0 for all) in ONE forward; instead of logits the
        pooled final hidden states come back: [n, dims] f32 for pooling "last" / "mean" / "first", [total tokens, dims] for "none"
        (dims = dimensions or the hidden size).  mask "full": every token sees its whole sequence; the caches must be empty, and are
        to be reset before anything decodes from them."""
        n = len(caches)
        assert len(seqs) == n
        ps = [np.ascontiguousarray(p, dtype=np.uint32).reshape(-1) for p in seqs]
        ids = np.ascontiguousarray(np.concatenate(ps) if ps else np.zeros(0, np.uint32), dtype=np.uint32)
        offsets = np.ascontiguousarray(np.concatenate([[0], np.cumsum([p.size for p in ps])]), dtype=np.uint64)
        pos = np.ascontiguousarray([0] * n if pos is None else pos, dtype=np.uint64)
        arr = (C.c_void_p * max(n, 1))(*[c._h for c in caches])
        st = make_embed(pooling, mask, normalize, dimensions)
        h = int(self.cfg["hidden_size"])
        dims = int(dimensions) if 0 < int(dimensions) <= h else h
        rows = int(offsets[-1]) if st.pooling == POOLING["none"] else n
        out = np.empty((max(rows, 1), dims), dtype=np.float32)
        _check(lib().fl_batch_embed(self._h, C.cast(arr, C.c_void_p), n, ids.ctypes.data, offsets.ctypes.data, pos.ctypes.data, C.byref(st),
                                    out.ctypes.data))
        return out[:rows]

    def forward_score(self, cache, ids, pos, top_n=0, targets=None, want_logits=False):
        """fl_forward_score: forward(cache, ids, pos) with every row scored on the device; nothing is selected.  targets None: row i's
        target is ids[i + 1], the last row has none; else [T] ids (SCORE_NO_TARGET: none).  Returns a ScoreResult; want_logits: with
        the [T, V] rows the kernel read (a diagnostic)."""
        ids = np.ascontiguousarray(ids, dtype=np.uint32)
        out = _ScoreArrays(ids.size, top_n, targets, self.V if want_logits else None)
        st = out.struct()
        _check(lib().fl_forward_score(self._h, cache._h, ids.ctypes.data, ids.size, pos, C.byref(st)))
        return out.result()

    def score_packed(self, caches, seqs, pos=None, top_n=0, targets=None, want_logits=False):
        """fl_batch_score: seqs[i] appended to caches[i] at RoPE offset pos[i] (None: 0 for all) in ONE forward, every row scored.
        targets None: next-token scoring per member (every member's last row has none); else one list of ids per member.  Returns one
        ScoreResult per member (views of the call's arrays)."""
        n = len(caches)
        assert len(seqs) == n
        ps = [np.ascontiguousarray(p, dtype=np.uint32).reshape(-1) for p in seqs]
        ids = np.ascontiguousarray(np.concatenate(ps) if ps else np.zeros(0, np.uint32), dtype=np.uint32)
        offsets = np.ascontiguousarray(np.concatenate([[0], np.cumsum([p.size for p in ps])]), dtype=np.uint64)
        pos = np.ascontiguousarray([0] * n if pos is None else pos, dtype=np.uint64)
        arr = (C.c_void_p * max(n, 1))(*[c._h for c in caches])
        tg = None if targets is None else np.concatenate([np.asarray(t, dtype=np.uint32).reshape(-1) for t in targets])
        out = _ScoreArrays(ids.size, top_n, tg, self.V if want_logits else None)
        st = out.struct()
        _check(lib().fl_batch_score(self._h, C.cast(arr, C.c_void_p), n, ids.ctypes.data, offsets.ctypes.data, pos.ctypes.data, C.byref(st)))
        r = out.result()
        cut = [slice(int(offsets[i]), int(offsets[i + 1])) for i in range(n)]
        return [ScoreResult(r.target_logprob[c], r.target_rank[c], r.top_ids[c], r.top_logprobs[c], None if r.logits is None else r.logits[c])
                for c in cut]

    def decode_sample(self, cache, first_token, pos, n_steps, temperature, seed=0, draws_done=1, eos=-1, top_p=None, top_k=None,
                      logprobs=None):
        """logprobs = N: returns (tokens, token_logprob [n], top_ids [n, N], top_logprobs [n, N]), n = the tokens emitted; a greedy
        decode with log-probs is temperature=0."""
        toks = np.zeros(max(n_steps, 1), dtype=np.uint32)
        n = C.c_size_t(0)
        if logprobs is not None:
            sp = make_sampler(temperature, seed, draws_done, top_p, top_k)
            lp = _LogprobArrays(n_steps, logprobs)
            st = lp.struct()
            _check(lib().fl_decode_sample_lp(self._h, cache._h, int(first_token), pos, n_steps, eos, C.byref(sp), toks.ctypes.data,
                                             C.byref(n), C.byref(st)))
            return (toks[: n.value],) + lp.cut(n.value)
        if top_p is not None or top_k is not None:
            sp = make_sampler(temperature, seed, draws_done, top_p, top_k)
            _check(lib().fl_decode_sample_ex(self._h, cache._h, int(first_token), pos, n_steps, eos, C.byref(sp), toks.ctypes.data,
                                             C.byref(n)))
            return toks[: n.value]
        sp = FlSampling(temperature, seed, draws_done)
        _check(lib().fl_decode_sample(self._h, cache._h, int(first_token), pos, n_steps, eos, C.byref(sp), toks.ctypes.data,
                                      C.byref(n)))
        return toks[: n.value]

    def synchronize(self):
        _check(lib().fl_synchronize(self._h))

    def ipc_export(self):
        """This rank's inbox handle (FL_TP_MULTI_PROCESS): ship it to every peer."""
        buf = C.create_string_buffer(IPC_HANDLE_BYTES)
        _check(lib().fl_comm_ipc_export(self._h, buf))
        return buf.raw

    def ipc_connect(self, handles):
        """handles: the tp handles in rank order (own one included)."""
        blob = b"".join(bytes(h) for h in handles)
        buf = C.create_string_buffer(blob, len(blob))
        _check(lib().fl_comm_ipc_connect(self._h, buf))

    def comm_probe(self, form, n, iters=64):
        """us per decode-sized all-reduce on this group's links: form 0 RCCL, 1 one-shot kernel, 2 fused into the GEMV epilogue
        (None: not available).  Collective: every rank calls it."""
        us = C.c_double(-1.0)
        _check(lib().fl_comm_probe(self._h, form, n, iters, C.byref(us)))
        return None if us.value < 0 else us.value

    def comm_selftest(self, n):
        """One all-reduce of n integer-valued floats over the connected inboxes, checked exactly (n >= 16384: the many-workgroup form).
        Collective: every rank calls it.  True: this rank holds the exact sums."""
        ok = C.c_int32(0)
        _check(lib().fl_comm_selftest(self._h, n, C.byref(ok)))
        return bool(ok.value)

    def profile_begin(self):
        _check(lib().fl_profile_begin(self._h))

    def profile_end(self):
        stats = (FlKernelStat * 64)()
        n = C.c_size_t(0)
        _check(lib().fl_profile_end(self._h, stats, 64, C.byref(n)))
        return [dict(name=stats[i].name.decode(), launches=stats[i].launches, total_ms=stats[i].total_ms,
                     bytes=stats[i].bytes, flops=stats[i].flops) for i in range(min(n.value, 64))]

    def close(self):
        if getattr(self, "_h", None):
            lib().fl_model_release(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Guide:
    """fl_guide: an immutable token-level automaton of one model (CSR: state s allows tokens[row_ptr[s]:row_ptr[s + 1]], tokens[e]
    leads to state next[e]), shareable by any number of its caches (Cache.set_guide)."""

    def __init__(self, model, row_ptr, tokens, next):
        st, keep = make_guide_desc(row_ptr, tokens, next)
        h = C.c_void_p()
        _check(lib().fl_guide_create(model._h, C.byref(st), C.byref(h)))
        del keep
        self._h = h
        self._model = model
        self.n_states = int(st.n_states)

    def close(self):
        """fl_guide_destroy: drops this handle's reference (a cache that has the guide installed keeps its own)."""
        if getattr(self, "_h", None):
            lib().fl_guide_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Batch:
    """fl_batch: up to 64 caches of one model decoded together."""

    def __init__(self, model, caches):
        self._model, self._caches = model, list(caches)
        arr = (C.c_void_p * len(caches))(*[c._h for c in caches])
        h = C.c_void_p()
        _check(lib().fl_batch_create(model._h, arr, len(caches), C.byref(h)))
        self._h = h
        self.n = len(caches)

    def forward(self, tokens, pos, want_logits=True):
        tokens = np.ascontiguousarray(tokens, dtype=np.uint32)
        pos = np.ascontiguousarray(pos, dtype=np.uint64)
        lg = np.empty((self.n, self._model.V), dtype=np.float32) if want_logits else None
        am = np.zeros(self.n, dtype=np.uint32)
        _check(lib().fl_batch_forward(self._h, tokens.ctypes.data, pos.ctypes.data, lg.ctypes.data if want_logits else None,
                                      am.ctypes.data))
        return (lg, am) if want_logits else am

    def replace(self, slot, cache):
        """Continuous batching: `cache` takes the place of sequence `slot` (the batch is not rebuilt)."""
        _check(lib().fl_batch_replace(self._h, slot, cache._h))
        self._caches[slot] = cache

    def decode(self, first_tokens, pos, n_steps, eos=-1, temperature=None, seed=0, draws_done=1):
        first = np.ascontiguousarray(first_tokens, dtype=np.uint32)
        pos = np.ascontiguousarray(pos, dtype=np.uint64)
        out = np.zeros((self.n, max(n_steps, 1)), dtype=np.uint32)
        n_out = np.zeros(self.n, dtype=np.uint64)
        sp = FlSampling(temperature, seed, draws_done) if temperature is not None else None
        _check(lib().fl_batch_decode(self._h, first.ctypes.data, pos.ctypes.data, n_steps, eos, C.byref(sp) if sp else None,
                                     out.ctypes.data, n_out.ctypes.data))
        return [out[i, : int(n_out[i])] for i in range(self.n)]

    def decode_each(self, first_tokens, pos, n_steps, eos=None, temperatures=None, seeds=None, draws_done=None, top_p=None, top_k=None,
                    logprobs=None):
        """fl_batch_decode_each: per-sequence EOS ids (None / negative: none) and temperatures (None / < 1e-7: ArgMax).  With top_p /
        top_k (lists, None entries: off) it is fl_batch_decode_each_ex: one batch mixes ArgMax, Sampling::All and top-p / top-k.
        logprobs (an int, or one per sequence): fl_batch_decode_each_lp; every sequence's entry is then (tokens, token_logprob,
        top_ids, top_logprobs)."""
        first = np.ascontiguousarray(first_tokens, dtype=np.uint32)
        pos = np.ascontiguousarray(pos, dtype=np.uint64)
        out = np.zeros((self.n, max(n_steps, 1)), dtype=np.uint32)
        n_out = np.zeros(self.n, dtype=np.uint64)
        e = np.ascontiguousarray([-1 if x is None else int(x) for x in (eos if eos is not None else [None] * self.n)], dtype=np.int64)
        if top_p is not None or top_k is not None or logprobs is not None:
            spx = (FlSampler * self.n)()
            for i in range(self.n):
                t = temperatures[i] if temperatures is not None and temperatures[i] is not None else 0.0
                spx[i] = make_sampler(t, seeds[i] if seeds is not None else 0, draws_done[i] if draws_done is not None else 1,
                                      top_p[i] if top_p is not None else None, top_k[i] if top_k is not None else None)
            if logprobs is not None:
                tops = [int(logprobs)] * self.n if np.isscalar(logprobs) else [int(x) for x in logprobs]
                lps = [_LogprobArrays(n_steps, tops[i]) for i in range(self.n)]
                lpx = (FlLogprobs * self.n)(*[x.struct() for x in lps])
                _check(lib().fl_batch_decode_each_lp(self._h, first.ctypes.data, pos.ctypes.data, n_steps, e.ctypes.data, C.cast(spx, C.c_void_p),
                                                     out.ctypes.data, n_out.ctypes.data, C.cast(lpx, C.c_void_p)))
                return [(out[i, : int(n_out[i])],) + lps[i].cut(int(n_out[i])) for i in range(self.n)]
            _check(lib().fl_batch_decode_each_ex(self._h, first.ctypes.data, pos.ctypes.data, n_steps, e.ctypes.data, C.cast(spx, C.c_void_p),
                                                 out.ctypes.data, n_out.ctypes.data))
            return [out[i, : int(n_out[i])] for i in range(self.n)]
        sp = (FlSampling * self.n)()
        for i in range(self.n):
            t = temperatures[i] if temperatures is not None and temperatures[i] is not None else 0.0
            sp[i] = FlSampling(t, seeds[i] if seeds is not None else 0, draws_done[i] if draws_done is not None else 1)
        _check(lib().fl_batch_decode_each(self._h, first.ctypes.data, pos.ctypes.data, n_steps, e.ctypes.data, C.cast(sp, C.c_void_p),
                                          out.ctypes.data, n_out.ctypes.data))
        return [out[i, : int(n_out[i])] for i in range(self.n)]

    def close(self):
        if getattr(self, "_h", None):
            lib().fl_batch_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Cache:
    def __init__(self, model, max_seq):
        h = C.c_void_p()
        _check(lib().fl_cache_create(model._h, max_seq, C.byref(h)))
        self._h = h
        self._model = model

    def reset(self):
        lib().fl_cache_reset(self._h)

    def truncate(self, n):
        """fl_cache_truncate: forget everything from position n on."""
        _check(lib().fl_cache_truncate(self._h, int(n)))

    def copy_prefix(self, src, n):
        """fl_cache_copy_prefix: this cache forgets what it holds and takes the first n cached positions of `src` (same model)."""
        _check(lib().fl_cache_copy_prefix(self._h, src._h if src is not None else None, int(n)))

    def set_logit_rules(self, prompt_ids=(), output_ids=(), logit_bias=None, repetition_penalty=1.0, frequency_penalty=0.0,
                        presence_penalty=0.0):
        """fl_cache_set_logit_rules: logit_bias {id: bias} (-inf bans an id) and the three penalties, applied on the device to every
        row this cache's calls select a token from; prompt_ids mark "seen in the prompt", output_ids seed the output counts, which
        the decode loops then keep themselves."""
        st, keep = make_logit_rules(logit_bias, repetition_penalty, frequency_penalty, presence_penalty)
        p = np.ascontiguousarray(prompt_ids, dtype=np.uint32).reshape(-1)
        o = np.ascontiguousarray(output_ids, dtype=np.uint32).reshape(-1)
        _check(lib().fl_cache_set_logit_rules(self._model._h, self._h, C.byref(st), p.ctypes.data if p.size else None, p.size,
                                              o.ctypes.data if o.size else None, o.size))
        del keep

    def clear_logit_rules(self):
        _check(lib().fl_cache_set_logit_rules(self._model._h, self._h, None, None, 0, None, 0))

    def logit_counts(self):
        """fl_cache_logit_counts: the table words uint32 [V] -- bit 31 "in the prompt", bits 0..30 the output count."""
        out = np.zeros(self._model.V, dtype=np.uint32)
        _check(lib().fl_cache_logit_counts(self._model._h, self._h, out.ctypes.data))
        return out

    def set_guide(self, guide, state=0):
        """fl_cache_set_guide: every token this cache's calls select comes from the list of the automaton's current state, and moves
        the cache along its edge.  truncate / reset / copy_prefix leave the state alone: set it again after a rollback."""
        _check(lib().fl_cache_set_guide(self._model._h, self._h, guide._h, int(state)))

    def clear_guide(self):
        _check(lib().fl_cache_set_guide(self._model._h, self._h, None, 0))

    def guide_state(self):
        """fl_cache_guide_state: the state in which the next selected token is looked up."""
        out = C.c_uint32(0)
        _check(lib().fl_cache_guide_state(self._h, C.byref(out)))
        return int(out.value)

    def __len__(self):
        return lib().fl_cache_len(self._h)

    def capacity(self):
        return lib().fl_cache_capacity(self._h)

    def close(self):
        if getattr(self, "_h", None):
            lib().fl_cache_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def tune(key, value):
    _check(lib().fl_tune(key.encode(), int(value)))


def reload_env():
    """The library reads its FL_<NAME> switches from the environment ONCE (first use); after changing os.environ in a live process
    call this to have every switch re-read."""
    _check(lib().fl_tune(b"reload_env", 0))


def library_loaded():
    return _LIB is not None


def op_attention(q, k, v, s_past, H, Hkv, d, window=-1, kernel=0, nsplit=0):
    """The bf16 MFMA attention kernels alone.  q [T, H*d], k / v [s_past + T, Hkv*d]: uint16 bf16 bits; returns [T, H*d] f32."""
    q, k, v = (np.ascontiguousarray(a, dtype=np.uint16) for a in (q, k, v))
    T = q.shape[0]
    assert q.shape == (T, H * d) and k.shape == (s_past + T, Hkv * d) and v.shape == k.shape
    out = np.empty((T, H * d), dtype=np.float32)
    _check(lib().fl_op_attention(q.ctypes.data, k.ctypes.data, v.ctypes.data, T, s_past, H, Hkv, d, window, kernel, nsplit, out.ctypes.data))
    return out


def _attn_dtype(*arrays):
    """uint16 arrays are bf16 bits, float32 arrays fp32: (FL_DTYPE code, numpy dtype) of a set of attention operands."""
    kinds = set(np.asarray(a).dtype for a in arrays)
    assert len(kinds) == 1 and kinds <= {np.dtype(np.uint16), np.dtype(np.float32)}, kinds
    dt = kinds.pop()
    return (1 if dt == np.uint16 else 0), dt


def op_attention_plain(q, k, v, s_past, H, Hkv, d, layout=0, kernel=0, call0=None, capacity=None, window=-1, nsplit=1, pad_value=0.0,
                       repeat=1):
    """The single-sequence attention launches on a cache built in the model's layout (fl_op_attention_plain): layout 0 = the plain
    (VALU) kernels, bf16 (uint16 bits) or float32 by the arrays' dtype; layout 1 = the bf16 MFMA kernels.  q [T, H*d]; k / v
    [rows, Hkv*d] with rows >= s_past + T (the rows behind s_past + T are stale cache contents); positions from rows to `capacity`
    hold pad_value.  Returns [repeat, T, H*d] f32: the output of every one of `repeat` launches on the same scratch."""
    code, dt = _attn_dtype(q, k, v)
    q, k, v = (np.ascontiguousarray(a, dtype=dt) for a in (q, k, v))
    T, rows = q.shape[0], k.shape[0]
    assert q.shape == (T, H * d) and k.shape == (rows, Hkv * d) and v.shape == k.shape
    out = np.empty((max(repeat, 1), T, H * d), dtype=np.float32)
    _check(lib().fl_op_attention_plain(q.ctypes.data, k.ctypes.data, v.ctypes.data, code, layout, kernel, T, s_past,
                                       s_past if call0 is None else call0, rows, rows if capacity is None else capacity, H, Hkv, d, window,
                                       nsplit, pad_value, repeat, out.ctypes.data))
    return out


def op_attention_batch(q, ks, vs, lens, seq_alloc, nsplit, H, Hkv, d, layout=0, layer=0, pad_value=0.0, repeat=1):
    """The batched decode attention launches alone (fl_op_attention_batch).  q [B, H*d]; ks[b] / vs[b] [n_layers, rows_b, Hkv*d]
    (uint16 bf16 bits or float32); lens[b] keys of layer `layer` are visible to sequence b, the rows behind are stale contents.
    seq_alloc[b]: the cache's row count (a multiple of 32); nsplit[b]: its split count (0: as fl_cache_create).  Returns
    [repeat, B, H*d] f32."""
    code, dt = _attn_dtype(q, *ks, *vs)
    q = np.ascontiguousarray(q, dtype=dt)
    ks = [np.ascontiguousarray(a, dtype=dt) for a in ks]
    vs = [np.ascontiguousarray(a, dtype=dt) for a in vs]
    B, n_layers = q.shape[0], ks[0].shape[0]
    assert q.shape == (B, H * d) and len(ks) == len(vs) == len(lens) == len(seq_alloc) == len(nsplit) == B
    for a, b in zip(ks, vs):
        assert a.ndim == 3 and a.shape[0] == n_layers and a.shape[2] == Hkv * d and a.shape == b.shape
    kp = (C.c_void_p * B)(*[a.ctypes.data for a in ks])
    vpp = (C.c_void_p * B)(*[a.ctypes.data for a in vs])
    i64 = lambda x: np.ascontiguousarray(x, dtype=np.int64)
    ln, rows, sa, ns = i64(lens), i64([a.shape[1] for a in ks]), i64(seq_alloc), np.ascontiguousarray(nsplit, dtype=np.int32)
    out = np.empty((max(repeat, 1), B, H * d), dtype=np.float32)
    _check(lib().fl_op_attention_batch(q.ctypes.data, C.cast(kp, C.c_void_p), C.cast(vpp, C.c_void_p), code, layout, B, ln.ctypes.data,
                                       rows.ctypes.data, sa.ctypes.data, ns.ctypes.data, n_layers, layer, H, Hkv, d, pad_value, repeat,
                                       out.ctypes.data))
    return out


def op_attention_packed(q, ks, vs, counts, s_past, seq_alloc, H, Hkv, d, layer=0, window=-1, pad_value=0.0, mask=0, ex=True):
    """The packed prefill attention launch alone (fl_op_attention_packed_ex; ex=False: fl_op_attention_packed, mask 0 only; bf16 bits,
    MFMA layout).  mask 1: every new token sees all of its sequence's keys, the window is ignored.  q [sum(counts), H*d], member s's
    rows back to back; ks[s] / vs[s] [n_layers, rows_s, Hkv*d]: rows [0, s_past[s]) its cached prefix, the next counts[s] its new
    tokens, the rest stale contents; seq_alloc[s]: its cache's row count (a multiple of 32).  Returns [sum(counts), H*d] f32."""
    q = np.ascontiguousarray(q, dtype=np.uint16)
    ks = [np.ascontiguousarray(a, dtype=np.uint16) for a in ks]
    vs = [np.ascontiguousarray(a, dtype=np.uint16) for a in vs]
    n, n_layers = len(ks), ks[0].shape[0]
    i64 = lambda x: np.ascontiguousarray(x, dtype=np.int64)
    off = i64(np.concatenate([[0], np.cumsum(counts)]))
    T = int(off[-1])
    assert q.shape == (T, H * d) and len(vs) == len(counts) == len(s_past) == len(seq_alloc) == n
    for a, b in zip(ks, vs):
        assert a.ndim == 3 and a.shape[0] == n_layers and a.shape[2] == Hkv * d and a.shape == b.shape
    kp = (C.c_void_p * n)(*[a.ctypes.data for a in ks])
    vpp = (C.c_void_p * n)(*[a.ctypes.data for a in vs])
    sp, rows, sa = i64(s_past), i64([a.shape[1] for a in ks]), i64(seq_alloc)
    out = np.empty((T, H * d), dtype=np.float32)
    if ex:
        _check(lib().fl_op_attention_packed_ex(q.ctypes.data, C.cast(kp, C.c_void_p), C.cast(vpp, C.c_void_p), n, off.ctypes.data, sp.ctypes.data,
                                               rows.ctypes.data, sa.ctypes.data, n_layers, layer, H, Hkv, d, window, pad_value, int(mask), out.ctypes.data))
        return out
    assert mask == 0
    _check(lib().fl_op_attention_packed(q.ctypes.data, C.cast(kp, C.c_void_p), C.cast(vpp, C.c_void_p), n, off.ctypes.data, sp.ctypes.data,
                                        rows.ctypes.data, sa.ctypes.data, n_layers, layer, H, Hkv, d, window, pad_value, out.ctypes.data))
    return out


def op_pool_rows(x, inv_rms, w, counts, pooling="last", normalize=False, dimensions=0, iters=0):
    """The pool launch of fl_batch_embed alone (fl_op_pool_rows): x [T, h] f32 residual rows, inv_rms [T], w [h]; member s owns
    counts[s] consecutive rows.  Returns [n, dims] f32 ([T, dims] for pooling "none"); iters > 0: the ms per pool instead
    (fl_op_pool_rows_time)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    inv_rms = np.ascontiguousarray(inv_rms, dtype=np.float32).reshape(-1)
    w = np.ascontiguousarray(w, dtype=np.float32).reshape(-1)
    T, h = x.shape
    off = np.ascontiguousarray(np.concatenate([[0], np.cumsum(counts)]), dtype=np.uint64)
    assert int(off[-1]) == T and inv_rms.size == T and w.size == h
    st = make_embed(pooling, 0, normalize, dimensions)
    if iters > 0:
        ms = C.c_double(0.0)
        _check(lib().fl_op_pool_rows_time(x.ctypes.data, inv_rms.ctypes.data, w.ctypes.data, off.ctypes.data, len(counts), h, C.byref(st), iters,
                                          C.byref(ms)))
        return ms.value
    dims = int(dimensions) if 0 < int(dimensions) <= h else h
    rows = T if st.pooling == POOLING["none"] else len(counts)
    out = np.empty((rows, dims), dtype=np.float32)
    _check(lib().fl_op_pool_rows(x.ctypes.data, inv_rms.ctypes.data, w.ctypes.data, off.ctypes.data, len(counts), h, C.byref(st), out.ctypes.data))
    return out


def op_kv_copy(src, dst, width_bytes, iters=0):
    """The K/V prefix copy kernel alone: the first width_bytes bytes of every row of src go to the same row of dst.  src, dst: 2-D
    uint8 arrays with the same number of rows, C-contiguous (their row lengths are the two pitches).  Returns the new dst (and the ms
    per launch when iters > 0); dst itself is not modified."""
    src = np.ascontiguousarray(src, dtype=np.uint8)
    out = np.array(dst, dtype=np.uint8, order="C", copy=True)
    assert src.ndim == 2 and out.ndim == 2 and src.shape[0] == out.shape[0]
    ms = C.c_double(0.0)
    _check(lib().fl_op_kv_copy(src.ctypes.data, out.ctypes.data, src.shape[0], int(width_bytes), src.shape[1], out.shape[1], iters,
                               C.byref(ms)))
    return (out, ms.value) if iters else out


def op_linear(x, w, bias=None, epilogue=0, iters=0):
    """y = x . w^T (+bias) through the projection kernels.  x [T,K], w [N,K]: both float32 or both uint16 (bf16)."""
    x = np.ascontiguousarray(x)
    w = np.ascontiguousarray(w)
    assert x.dtype == w.dtype
    T, K = x.shape
    N = w.shape[0]
    y = np.empty((T, N // 2 if epilogue == 1 else N), dtype=np.float32)
    b = np.ascontiguousarray(bias, dtype=np.float32) if bias is not None else None
    ms = C.c_double(0.0)
    _check(lib().fl_op_linear(x.ctypes.data, w.ctypes.data, b.ctypes.data if b is not None else None, T, N, K,
                              _np_dtype_code(x), epilogue, y.ctypes.data, iters, C.byref(ms)))
    return (y, ms.value) if iters else y



def op_quantize_rows(w):
    """The FP8 row quantiser (device kernel) on a host matrix w [N,K], float32 or uint16 (bf16 bits): returns (q uint8 [N,K] of
    e4m3fn codes, s float32 [N] power-of-two row scales)."""
    w = np.ascontiguousarray(w)
    N, K = w.shape
    q = np.empty((N, K), dtype=np.uint8)
    s = np.empty(N, dtype=np.float32)
    _check(lib().fl_op_quantize_rows(w.ctypes.data, _np_dtype_code(w), N, K, q.ctypes.data, s.ctypes.data))
    return q, s


def op_gemv_w8(x, q, s, bias=None, epilogue=0, iters=0):
    """y[N] = s * (q . x) (+bias) through the FP8 decode weight stream.  x [K] uint16 (bf16 bits), q [N,K] uint8 (e4m3fn), s [N]
    float32; epilogue 1: rows are gate | up in HF order, y is [N/2]."""
    x = np.ascontiguousarray(x, dtype=np.uint16)
    q = np.ascontiguousarray(q, dtype=np.uint8)
    s = np.ascontiguousarray(s, dtype=np.float32)
    N, K = q.shape
    assert x.shape == (K,) and s.shape == (N,)
    y = np.empty(N // 2 if epilogue == 1 else N, dtype=np.float32)
    b = np.ascontiguousarray(bias, dtype=np.float32) if bias is not None else None
    ms = C.c_double(0.0)
    _check(lib().fl_op_gemv_w8(x.ctypes.data, q.ctypes.data, s.ctypes.data, b.ctypes.data if b is not None else None, N, K,
                               epilogue, y.ctypes.data, iters, C.byref(ms)))
    return (y, ms.value) if iters else y


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _ptr(a):
    return a.ctypes.data if a is not None else None


def op_rmsnorm_add(x_res, delta, w, eps, dtype):
    """launch_rmsnorm_add alone (fl_op_rmsnorm_add).  x_res [T, h] float32; delta [n_slab, T, h] float32 or None; w [h]; dtype "bf16"
    or "f32": the type xs is rounded to.  Returns (the updated x_res, xs widened to float32, inv_rms [T])."""
    x = np.array(x_res, dtype=np.float32, order="C", copy=True)
    T, h = x.shape
    d = _f32(delta) if delta is not None else None
    assert d is None or d.shape[1:] == (T, h)
    w = _f32(w)
    assert w.shape == (h,)
    xs, inv = np.empty((T, h), np.float32), np.empty(T, np.float32)
    _check(lib().fl_op_rmsnorm_add(x.ctypes.data, _ptr(d), 0 if d is None else d.shape[0], w.ctypes.data, eps, T, h,
                                   BF16 if dtype == "bf16" else F32, xs.ctypes.data, inv.ctypes.data))
    return x, xs, inv


def op_norm_linear(form, w, norm_w=None, eps=0.0, x_res=None, delta=None, embed=None, tokens=None, x=None, bias=None, w_scale=None,
                   epilogue=0, pro=1, dtype=None, repeat=1):
    """Residual add -> RMSNorm -> one projection in the fused form `form` (fl_op_norm_linear; 0: rmsnorm_add + launch_linear with the
    row scale, 1: the single-sequence stream's norm prologue, 2: the same over FP8 weights (w uint8 [N, K] + w_scale), 3: the batched
    stream; pro=0 (form 3): no norm, x [T, K] uint16 instead).  w [N, K] float32 or uint16 (bf16 bits); x_res [T, K] float32 with
    delta [n_slab, T, K] or None -- or embed [V, K] (w's dtype) with tokens [T].  Returns (y, x_out or None, kernels [4])."""
    w = np.ascontiguousarray(w)
    N, K = w.shape
    code = (BF16 if dtype == "bf16" else F32) if dtype is not None else (BF16 if form == 2 else _np_dtype_code(w))
    a = FlNormLinearArgs()
    a.struct_size = C.sizeof(FlNormLinearArgs)
    a.form, a.dtype, a.epilogue, a.pro, a.repeat, a.eps = form, code, epilogue, pro, repeat, eps
    keep = [w]
    if embed is not None:
        embed = np.ascontiguousarray(embed)
        tokens = np.ascontiguousarray(tokens, dtype=np.uint32)
        T = tokens.shape[0]
        a.embed, a.tokens, a.vocab = embed.ctypes.data, tokens.ctypes.data, embed.shape[0]
        assert embed.shape[1] == K
    elif pro == 0:
        x = np.ascontiguousarray(x, dtype=np.uint16)
        T = x.shape[0]
        a.x = x.ctypes.data
    else:
        x_res = _f32(x_res)
        T = x_res.shape[0]
        assert x_res.shape == (T, K)
        a.x_res = x_res.ctypes.data
    keep += [embed, tokens, x, x_res]
    if delta is not None:
        delta = _f32(delta)
        assert delta.shape[1:] == (T, K)
        a.delta, a.n_slab = delta.ctypes.data, delta.shape[0]
    norm_w = _f32(norm_w) if norm_w is not None else None
    bias = _f32(bias) if bias is not None else None
    w_scale = _f32(w_scale) if w_scale is not None else None
    a.norm_w, a.bias, a.w_scale, a.w = _ptr(norm_w), _ptr(bias), _ptr(w_scale), w.ctypes.data
    a.T, a.N, a.K = T, N, K
    y = np.empty((T, N // 2 if epilogue == 1 else N), np.float32)
    x_out = np.empty((T, K), np.float32) if pro == 1 else None
    kernels = np.zeros(4, np.int32)
    a.y, a.x_out, a.kernels_out = y.ctypes.data, _ptr(x_out), kernels.ctypes.data
    keep += [delta, norm_w, bias, w_scale]
    _check(lib().fl_op_norm_linear(C.byref(a)))
    return y, x_out, kernels


def op_linear_resid(x, w, h_in, w_next, eps, bias=None, w2=None, epi2=0, lazy=False, repeat=1):
    """A bf16 projection with the residual + next-norm epilogue, and optionally the projection that consumes it (fl_op_linear_resid).
    x [T, K], w [N, K], w2 [N2, N]: uint16 (bf16 bits); h_in [T, N], w_next [N] float32.  Returns a dict: h, xn (widened), inv_rms,
    part [T, np], y2 (or None) and kernels = {kernel, ks, tail, tail_ks, consumer, consumer_reads_parts} (names of LK_NAMES)."""
    x, w = np.ascontiguousarray(x, dtype=np.uint16), np.ascontiguousarray(w, dtype=np.uint16)
    h_in, w_next = _f32(h_in), _f32(w_next)
    (T, K), N = x.shape, w.shape[0]
    assert w.shape == (N, K) and h_in.shape == (T, N) and w_next.shape == (N,)
    bias = _f32(bias) if bias is not None else None
    w2 = np.ascontiguousarray(w2, dtype=np.uint16) if w2 is not None else None
    a = FlLinearResidArgs()
    a.struct_size = C.sizeof(FlLinearResidArgs)
    a.T, a.N, a.K, a.N2 = T, N, K, 0 if w2 is None else w2.shape[0]
    a.x, a.w, a.bias, a.h_in, a.w_next, a.w2 = x.ctypes.data, w.ctypes.data, _ptr(bias), h_in.ctypes.data, w_next.ctypes.data, _ptr(w2)
    a.eps, a.lazy, a.epi2, a.repeat = eps, int(bool(lazy)), epi2, repeat
    np_ = (N + 255) // 256 * 4
    h, xn, inv, part = np.empty((T, N), np.float32), np.empty((T, N), np.float32), np.empty(T, np.float32), np.empty((T, np_), np.float32)
    y2 = np.empty((T, w2.shape[0] // 2 if epi2 == 1 else w2.shape[0]), np.float32) if w2 is not None else None
    kernels = np.zeros(6, np.int32)
    a.h_out, a.xn_out, a.inv_rms_out, a.part_out, a.y2_out, a.kernels_out = (h.ctypes.data, xn.ctypes.data, inv.ctypes.data, part.ctypes.data,
                                                                               _ptr(y2), kernels.ctypes.data)
    _check(lib().fl_op_linear_resid(C.byref(a)))
    k = dict(kernel=LK_NAMES[kernels[0]], ks=int(kernels[1]), tail=LK_NAMES[kernels[2]], tail_ks=int(kernels[3]), consumer=LK_NAMES[kernels[4]],
             consumer_reads_parts=bool(kernels[5]))
    return dict(h=h, xn=xn, inv_rms=inv, part=part, y2=y2, kernels=k)


def op_gemv_resid(mode, eps, x=None, w=None, h_in=None, w_next=None, xs=None, cs=None, w2=None, epi2=0, rope=None, repeat=1):
    """The decode stream's residual epilogue and the prologue that consumes it (fl_op_gemv_resid).  mode 0: the producer alone
    (x [K], w [N, K] uint16 bf16 bits; h_in, w_next [N] float32); 1: the consumer alone on xs [N] (uint16) and cs [N/8] with w2
    [N2, N]; 2: the pair next to today's two launches.  epi2: 0 fp32 (+ ArgMax candidates), 1 gate/up (w2 rows gate | up), 2 QKV
    RoPE with rope = dict(H, Hkv, d, pos, len, seq_alloc, cos, sin) (cos / sin [max_pos, d/2] float32).  Returns a dict of what the mode
    gives: h, xs (uint16), cs, delta (the producer's untouched `out`), y, inv, amax, and h_ref, y_ref, inv_ref, amax_ref (mode 2)."""
    keep = []

    def u16(v):
        v = None if v is None else np.ascontiguousarray(v, dtype=np.uint16)
        keep.append(v)
        return v

    def f32(v):
        v = None if v is None else _f32(v)
        keep.append(v)
        return v
    x, w, xs, w2 = u16(x), u16(w), u16(xs), u16(w2)
    h_in, w_next, cs = f32(h_in), f32(w_next), f32(cs)
    a = FlGemvResidArgs()
    a.struct_size = C.sizeof(FlGemvResidArgs)
    a.mode, a.epi2, a.repeat, a.eps = mode, epi2, repeat, eps
    N = w.shape[0] if w is not None else xs.shape[0]
    a.N, a.K, a.N2 = N, (w.shape[1] if w is not None else 0), (w2.shape[0] if w2 is not None else 0)
    assert w is None or (x.shape == (w.shape[1],) and h_in.shape == (N,) and w_next.shape == (N,))
    assert w2 is None or w2.shape[1] == N
    assert xs is None or (xs.shape == (N,) and cs.shape == (N // 8,))
    a.x, a.w, a.h_in, a.w_next, a.xs, a.cs, a.w2 = _ptr(x), _ptr(w), _ptr(h_in), _ptr(w_next), _ptr(xs), _ptr(cs), _ptr(w2)
    if rope is not None:
        cos, sin = f32(rope["cos"]), f32(rope["sin"])
        a.H, a.Hkv, a.d, a.pos, a.len, a.seq_alloc, a.max_pos = rope["H"], rope["Hkv"], rope["d"], rope["pos"], rope["len"], rope["seq_alloc"], cos.shape[0]
        a.cos_tab, a.sin_tab = cos.ctypes.data, sin.ctypes.data
    out = {}
    if mode != 1:
        out.update(h=np.empty(N, np.float32), xs=np.empty(N, np.uint16), cs=np.empty(N // 8, np.float32), delta=np.empty(N, np.float32))
        a.h_out, a.xs_out, a.cs_out, a.delta_out = (out[k].ctypes.data for k in ("h", "xs", "cs", "delta"))
    amax = np.full(2, -2, np.int32)
    if mode != 0:
        ny = a.N2 // 2 if epi2 == 1 else a.N2
        out.update(y=np.empty(ny, np.float32), inv=np.empty(1, np.float32))
        a.y_out, a.inv_out, a.amax_out = out["y"].ctypes.data, out["inv"].ctypes.data, amax.ctypes.data
        if mode == 2:
            out.update(h_ref=np.empty(N, np.float32), y_ref=np.empty(ny, np.float32), inv_ref=np.empty(1, np.float32))
            a.h_ref, a.y_ref, a.inv_ref = out["h_ref"].ctypes.data, out["y_ref"].ctypes.data, out["inv_ref"].ctypes.data
    _check(lib().fl_op_gemv_resid(C.byref(a)))
    if mode != 0:
        out.update(amax=int(amax[0]), amax_ref=int(amax[1]))
    return out


def _rope_seqs(st, seqs, layers, layer, bf16):
    """fill an FlRopeSeqs from a list of dicts (count, pos, len, seq_alloc, vt, k, v); k / v: the whole caches, uint16 (bf16 bits) or
    float32.  Returns (the copies of the caches that the call updates, arrays to keep alive)."""
    n = len(seqs)
    cols = [np.array([int(s[key]) for s in seqs], dtype=np.int32) for key in ("count", "pos", "len", "seq_alloc", "vt")]
    et = np.uint16 if bf16 else np.float32
    ks = [np.array(s["k"], dtype=et, order="C", copy=True) for s in seqs]
    vs = [np.array(s["v"], dtype=et, order="C", copy=True) for s in seqs]
    kp = (C.c_void_p * n)(*[a.ctypes.data for a in ks])
    vp = (C.c_void_p * n)(*[a.ctypes.data for a in vs])
    st.n_seq, st.layers, st.layer = n, layers, layer
    st.count, st.pos, st.len, st.seq_alloc, st.v_transposed = (c.ctypes.data for c in cols)
    st.k_cache, st.v_cache = C.addressof(kp), C.addressof(vp)
    return list(zip(ks, vs)), (cols, kp, vp)


def op_rope_kv(form, qkv, cos, sin, H, Hkv, d, seqs, dtype, bias=None, layers=1, layer=0, repeat=1):
    """The stand-alone RoPE + KV-append kernels (fl_op_rope_kv; form 0: launch_rope_kv, 1: launch_rope_kv_batch, 2:
    launch_rope_kv_packed).  qkv [n_slab, rows, (H + 2 Hkv) d] float32; cos / sin [max_pos, d / 2] float32; seqs: a list of dicts
    (count, pos, len, seq_alloc, vt, k, v) with the whole caches k / v [layers, Hkv, seq_alloc, d] (v [layers, Hkv, d, seq_alloc] where
    vt) as uint16 bf16 bits or float32 -- they are not modified.  Returns (q [rows, H d] as bits of dtype, [(k, v)] after the call,
    kernels [4] with kernels[0] an index into ROPE_KV_NAMES)."""
    bf16 = dtype == "bf16"
    qkv, cos, sin = _f32(qkv), _f32(cos), _f32(sin)
    n_slab, rows, N = qkv.shape
    assert N == (H + 2 * Hkv) * d and cos.shape == sin.shape and cos.shape[1] == d // 2
    bias = _f32(bias) if bias is not None else None
    a = FlRopeKvArgs()
    a.struct_size = C.sizeof(FlRopeKvArgs)
    a.form, a.dtype, a.n_slab, a.repeat = form, BF16 if bf16 else F32, n_slab, repeat
    a.H, a.Hkv, a.d, a.max_pos = H, Hkv, d, cos.shape[0]
    a.qkv, a.bias, a.cos_tab, a.sin_tab = qkv.ctypes.data, _ptr(bias), cos.ctypes.data, sin.ctypes.data
    caches, keep = _rope_seqs(a.seqs, seqs, layers, layer, bf16)
    q = np.empty((rows, H * d), np.uint16 if bf16 else np.float32)
    kernels = np.zeros(4, np.int32)
    a.q_out, a.kernels_out = q.ctypes.data, kernels.ctypes.data
    _check(lib().fl_op_rope_kv(C.byref(a)))
    del keep
    return q, caches, kernels


def op_qkv_rope(form, w, norm_w, eps, cos, sin, H, Hkv, d, seqs, dtype, x_res=None, delta=None, embed=None, tokens=None, bias=None,
                w_scale=None, layers=1, layer=0, repeat=1):
    """Residual add -> RMSNorm -> QKV projection with RoPE and the KV append behind it (fl_op_qkv_rope; form 0: the prompt path by
    plan_qkv_rope, 1: the single-sequence stream, 2: the same over FP8 weights (w uint8 + w_scale), 3: the batched stream).  w [N, K]
    in dtype; the norm's inputs as op_norm_linear; cos / sin / seqs as op_rope_kv.  Returns (q [T, H d] as bits of dtype, [(k, v)]
    after the call, x_out [T, K], kernels [4])."""
    bf16 = dtype == "bf16"
    w = np.ascontiguousarray(w)
    N, K = w.shape
    cos, sin, norm_w = _f32(cos), _f32(sin), _f32(norm_w)
    assert N == (H + 2 * Hkv) * d and cos.shape == sin.shape and cos.shape[1] == d // 2 and norm_w.shape == (K,)
    a = FlQkvRopeArgs()
    a.struct_size = C.sizeof(FlQkvRopeArgs)
    a.form, a.dtype, a.repeat, a.eps = form, BF16 if bf16 else F32, repeat, eps
    a.K, a.H, a.Hkv, a.d, a.max_pos = K, H, Hkv, d, cos.shape[0]
    if embed is not None:
        embed = np.ascontiguousarray(embed)
        tokens = np.ascontiguousarray(tokens, dtype=np.uint32)
        T = tokens.shape[0]
        assert embed.shape[1] == K
        a.embed, a.tokens, a.vocab = embed.ctypes.data, tokens.ctypes.data, embed.shape[0]
    else:
        x_res = _f32(x_res)
        T = x_res.shape[0]
        assert x_res.shape == (T, K)
        a.x_res = x_res.ctypes.data
    if delta is not None:
        delta = _f32(delta)
        assert delta.shape[1:] == (T, K)
        a.delta, a.n_slab = delta.ctypes.data, delta.shape[0]
    bias = _f32(bias) if bias is not None else None
    w_scale = _f32(w_scale) if w_scale is not None else None
    a.T, a.w, a.norm_w, a.bias, a.w_scale, a.cos_tab, a.sin_tab = T, w.ctypes.data, norm_w.ctypes.data, _ptr(bias), _ptr(w_scale), cos.ctypes.data, sin.ctypes.data
    caches, keep = _rope_seqs(a.seqs, seqs, layers, layer, bf16)
    q = np.empty((T, H * d), np.uint16 if bf16 else np.float32)
    x_out = np.empty((T, K), np.float32)
    kernels = np.zeros(4, np.int32)
    a.q_out, a.x_out, a.kernels_out = q.ctypes.data, x_out.ctypes.data, kernels.ctypes.data
    _check(lib().fl_op_qkv_rope(C.byref(a)))
    del keep
    return q, caches, x_out, kernels


def op_attn_oproj_rep(q, k, v, w_o, s_past, H, Hkv, d, capacity=None, pad_value=0.0, repeat=1):
    """Decode attention replicated inside the o_proj launch, alone (fl_op_attn_oproj_rep): q [H d], k / v [rows, Hkv d] with rows >
    s_past (the rows behind s_past + 1 are stale cache contents), w_o [N, H d], all uint16 bf16 bits; positions from rows to
    `capacity` hold pad_value.  Returns (out [repeat, N] float32: the output of every launch, info [6] = (model rule, any-size
    rule, rows per wave, GMAX, workgroups, slices per kv head))."""
    q, k, v, w_o = (np.ascontiguousarray(a, dtype=np.uint16) for a in (q, k, v, w_o))
    rows, N = k.shape[0], w_o.shape[0]
    assert q.size == H * d and k.shape == (rows, Hkv * d) and v.shape == k.shape and w_o.shape == (N, H * d)
    a = FlAttnOprojRepArgs()
    a.struct_size = C.sizeof(FlAttnOprojRepArgs)
    a.H, a.Hkv, a.d, a.N, a.s_past, a.k_rows, a.capacity = H, Hkv, d, N, s_past, rows, rows if capacity is None else capacity
    a.q, a.k, a.v, a.w_o, a.pad_value, a.repeat = q.ctypes.data, k.ctypes.data, v.ctypes.data, w_o.ctypes.data, pad_value, repeat
    out = np.empty((max(repeat, 1), N), dtype=np.float32)
    info = np.zeros(6, np.int32)
    a.out, a.info_out = out.ctypes.data, info.ctypes.data
    _check(lib().fl_op_attn_oproj_rep(C.byref(a)))
    return out, info


def op_attn_oproj_rep_info(H, Hkv, d, N, capacity):
    """info [6] of op_attn_oproj_rep for a shape and a cache capacity, without a device (query_only); FastLLMError for a head shape
    the kernel does not take."""
    a = FlAttnOprojRepArgs()
    a.struct_size = C.sizeof(FlAttnOprojRepArgs)
    a.H, a.Hkv, a.d, a.N, a.capacity, a.query_only = H, Hkv, d, N, capacity, 1
    info = np.zeros(6, np.int32)
    a.info_out = info.ctypes.data
    _check(lib().fl_op_attn_oproj_rep(C.byref(a)))
    return info
