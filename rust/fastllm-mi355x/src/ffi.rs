//! Raw FFI of `include/fastllm_mi355x.h` (ABI version 2).  One `#[repr(C)]` struct per C struct, one declaration per
//! entry point, same order as the header.  Every entry point returns an `fl_status` (`0` = OK) unless noted; none of
//! them unwinds (the library is an exception barrier), so calling them from Rust is sound.
#![allow(non_camel_case_types)]

use std::os::raw::{c_char, c_int, c_void};

pub const FL_ABI_VERSION: c_int = 2;
pub const FL_UNIQUE_ID_BYTES: usize = 128;
pub const FL_IPC_HANDLE_BYTES: usize = 64;
/// Most drafted ids one `fl_forward_verify` call scores (T = n_draft + 1 <= 16).
pub const FL_VERIFY_MAX_DRAFT: usize = 15;
pub const FL_LOGPROBS_MAX_TOP: usize = 20;

// fl_status
pub const FL_OK: c_int = 0;
pub const FL_ERR_BAD_CONFIG: c_int = -1;
pub const FL_ERR_MISSING_TENSOR: c_int = -2;
pub const FL_ERR_SHAPE_MISMATCH: c_int = -3;
pub const FL_ERR_OOM: c_int = -4;
pub const FL_ERR_HIP: c_int = -5;
pub const FL_ERR_RCCL: c_int = -6;
pub const FL_ERR_SEQ_OVERFLOW: c_int = -7;
pub const FL_ERR_BAD_ARGUMENT: c_int = -8;
pub const FL_ERR_NO_DEVICE: c_int = -9;
pub const FL_ERR_UNSUPPORTED: c_int = -10;

// fl_family (ModelArchitecture::get_family: llama.rs:153, mistral.rs:240, qwen.rs:174)
pub const FL_FAMILY_LLAMA: i32 = 0;
pub const FL_FAMILY_MISTRAL: i32 = 1;
pub const FL_FAMILY_QWEN2: i32 = 2;

// fl_dtype (candle_core::DType subset, dtype_utils.rs:10-23)
pub const FL_DTYPE_F32: i32 = 0;
pub const FL_DTYPE_BF16: i32 = 1;
pub const FL_DTYPE_F16: i32 = 2;

// fl_tp_mode
pub const FL_TP_NONE: i32 = 0;
pub const FL_TP_SINGLE_PROCESS: i32 = 1;
pub const FL_TP_MULTI_PROCESS: i32 = 2;
pub const FL_TP_EMULATED: i32 = 3;

// fl_weight_format: what the decode step streams (E4M3_ROW: e4m3fn weights with one power-of-two fp32 scale per output row)
pub const FL_WEIGHTS_COMPUTE_DTYPE: i32 = 0;
pub const FL_WEIGHTS_E4M3_ROW: i32 = 1;

// fl_activation: the encoder's GELU form (TANH: candle's Tensor::gelu, what the reference runs; ERF: the exact form HF BERT checkpoints were trained with)
pub const FL_ACT_GELU_TANH: i32 = 0;
pub const FL_ACT_GELU_ERF: i32 = 1;

/// `fl_config`: the fields of the reference's ConfigFile / BaseModelConfig (config.rs:6-18).  0 in an optional field
/// = absent from config.json = the reference's default.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct fl_config {
    pub family: i32,
    pub qkv_bias: i32,
    pub hidden_size: i64,
    pub intermediate_size: i64,
    pub vocab_size: i64,
    pub num_hidden_layers: i64,
    pub num_attention_heads: i64,
    pub num_key_value_heads: i64,
    pub max_position_embeddings: i64,
    pub sliding_window: i64,
    pub rms_norm_eps: f64,
    pub rope_theta: f64,
}

/// `fl_tensor`: one entry of initialize_model's `HashMap<String, Tensor>`; borrowed for the call only.
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct fl_tensor {
    pub name: *const c_char,
    pub dtype: i32,
    pub ndim: i32,
    pub shape: [i64; 4],
    pub data: *const c_void,
    pub device: i32,
    pub _pad: i32,
}

#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct fl_parallel {
    pub mode: i32,
    pub tp_size: i32,
    pub tp_rank: i32,
    pub n_device_ids: i32,
    pub device_ids: *const i32,
    pub unique_id: *const c_void,
}

#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct fl_model_info {
    pub cfg: fl_config,
    pub head_dim: i64,
    pub compute_dtype: i32,
    pub tp_size: i32,
    pub weight_bytes_per_token: i64,
    pub kv_bytes_per_position: i64,
    pub hbm_bytes_allocated: i64,
    pub small_collectives: i32,
    pub fused_all_reduce: i32,
    pub rccl_ranks: i32,
    pub decode_weights: i32,
}

/// `fl_model_options` (fl_model_create_opts): `struct_size` must be `size_of::<fl_model_options>()`.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct fl_model_options {
    pub struct_size: u32,
    pub decode_weights: i32,
    pub _reserved: [i64; 3],
}

/// `fl_sampling`: LogitsProcessor::new(seed, Some(temperature), None) (mod.rs:373-374).
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct fl_sampling {
    pub temperature: f64,
    pub seed: u64,
    pub draws_done: u64,
}

/// `fl_sampler`: temperature + top_p + top_k (candle's Sampling::TopP / TopK / TopKThenTopP); `struct_size` is
/// `size_of::<fl_sampler>()`.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct fl_sampler {
    pub struct_size: u32,
    pub top_k: i32,
    pub temperature: f64,
    pub top_p: f64,
    pub seed: u64,
    pub draws_done: u64,
    pub _reserved: [i64; 2],
}

/// `fl_logprobs`: where the log-probabilities of an `fl_*_lp` call go -- the chosen token's per step and, with `top_n > 0`, the
/// `top_n` most likely tokens' ids and values (host arrays of n and n x top_n entries); `struct_size` is `size_of::<fl_logprobs>()`.
/// The distribution is the model's own (temperature 1, nothing masked), whatever sampler chose the token.
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct fl_logprobs {
    pub struct_size: u32,
    pub top_n: i32,
    pub token_logprob: *mut f32,
    pub top_ids: *mut u32,
    pub top_logprobs: *mut f32,
    pub _reserved: [i64; 2],
}

/// `FL_SCORE_NO_TARGET`: a row of a scoring call without a target.
pub const FL_SCORE_NO_TARGET: u32 = 4294967295;

/// `fl_score`: what a scoring call (`fl_forward_score`, `fl_batch_score`) scores every row against and where the results go -- host
/// arrays over the call's T rows.  `targets` null: next-token scoring (row i's target is `ids[i + 1]`, a sequence's last row has none).
/// `target_rank` and `logits_out` (a diagnostic, `[T][V]`) are optional; `struct_size` is `size_of::<fl_score>()`.
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct fl_score {
    pub struct_size: u32,
    pub top_n: i32,
    pub targets: *const u32,
    pub target_logprob: *mut f32,
    pub target_rank: *mut u32,
    pub top_ids: *mut u32,
    pub top_logprobs: *mut f32,
    pub logits_out: *mut f32,
    pub _reserved: [i64; 2],
}

/// `fl_pooling`: which of a member's rows a decoder-model embedding call (`fl_batch_embed`) returns.
pub const FL_POOL_LAST: i32 = 0;
pub const FL_POOL_MEAN: i32 = 1;
pub const FL_POOL_FIRST: i32 = 2;
pub const FL_POOL_NONE: i32 = 3;
/// `fl_attn_mask`: causal (with the model's sliding window) or full -- every token sees its whole sequence, no window.
pub const FL_MASK_CAUSAL: i32 = 0;
pub const FL_MASK_FULL: i32 = 1;

/// `fl_embed`: the options of `fl_batch_embed` (and `fl_op_pool_rows`); `struct_size` is `size_of::<fl_embed>()`.  `dimensions` 0 is
/// the hidden size; otherwise the first `dimensions` columns are kept and THEN normalised.
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct fl_embed {
    pub struct_size: u32,
    pub pooling: i32,
    pub mask: i32,
    pub normalize: i32,
    pub dimensions: i64,
    pub _reserved: [i64; 2],
}

/// `fl_logit_rules`: `logit_bias` entries and the repetition / frequency / presence penalties a cache applies on the device to every
/// row it selects a token from (fl_cache_set_logit_rules); `struct_size` is `size_of::<fl_logit_rules>()`.  `repetition_penalty` 1 and
/// the other two 0 are off; a bias of negative infinity bans an id.
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct fl_logit_rules {
    pub struct_size: u32,
    pub n_bias: u32,
    pub bias_ids: *const u32,
    pub bias_values: *const f32,
    pub repetition_penalty: f32,
    pub frequency_penalty: f32,
    pub presence_penalty: f32,
    pub _reserved: [i64; 2],
}

/// `fl_guide_desc`: a token-level automaton in CSR form (fl_guide_create); `struct_size` is `size_of::<fl_guide_desc>()`.  State `s`
/// allows `tokens[row_ptr[s] .. row_ptr[s + 1]]` (strictly ascending, below the vocabulary), and `tokens[e]` leads to `next[e]`.
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct fl_guide_desc {
    pub struct_size: u32,
    pub n_states: u32,
    pub row_ptr: *const u64,
    pub tokens: *const u32,
    pub next: *const u32,
    pub _reserved: [i64; 2],
}

// kernel codes in the kernels_out arrays of fl_op_norm_linear / fl_op_linear_resid
pub const FL_LK_NONE: i32 = 0;
pub const FL_LK_GEMV: i32 = 1;
pub const FL_LK_H4: i32 = 2;
pub const FL_LK_W14: i32 = 3;
pub const FL_LK_SKF: i32 = 4;
pub const FL_LK_DMA: i32 = 5;
pub const FL_LK_SKINNY: i32 = 6;
pub const FL_LK_8P: i32 = 7;
pub const FL_LK_8P_STREAMK: i32 = 8;
pub const FL_LK_256: i32 = 9;
pub const FL_LK_128: i32 = 10;
pub const FL_LK_4W_ROPE: i32 = 11;
pub const FL_LK_GENERIC: i32 = 12;
pub const FL_LK_F32_ROWS: i32 = 13;
pub const FL_LK_F32_MFMA: i32 = 14;

/// `fl_norm_linear_args`: residual add -> RMSNorm -> one projection in a named fused form (fl_op_norm_linear, unit tests);
/// `struct_size` is `size_of::<fl_norm_linear_args>()`.
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct fl_norm_linear_args {
    pub struct_size: usize,
    pub form: i32,
    pub dtype: i32,
    pub epilogue: i32,
    pub pro: i32,
    pub t: i64,
    pub n: i64,
    pub k: i64,
    pub x_res: *const f32,
    pub x: *const c_void,
    pub delta: *const f32,
    pub norm_w: *const f32,
    pub embed: *const c_void,
    pub tokens: *const u32,
    pub w: *const c_void,
    pub w_scale: *const f32,
    pub bias: *const f32,
    pub vocab: i64,
    pub n_slab: i32,
    pub repeat: i32,
    pub eps: f32,
    pub reserved: f32,
    pub y: *mut f32,
    pub x_out: *mut f32,
    pub kernels_out: *mut i32,
}

/// `fl_linear_resid_args`: a projection with the residual + next-norm epilogue and, optionally, its consumer (fl_op_linear_resid,
/// unit tests); `struct_size` is `size_of::<fl_linear_resid_args>()`.
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct fl_linear_resid_args {
    pub struct_size: usize,
    pub t: i64,
    pub n: i64,
    pub k: i64,
    pub n2: i64,
    pub x: *const c_void,
    pub w: *const c_void,
    pub bias: *const f32,
    pub h_in: *const f32,
    pub w_next: *const f32,
    pub w2: *const c_void,
    pub eps: f32,
    pub lazy: i32,
    pub epi2: i32,
    pub repeat: i32,
    pub h_out: *mut f32,
    pub xn_out: *mut f32,
    pub inv_rms_out: *mut f32,
    pub part_out: *mut f32,
    pub y2_out: *mut f32,
    pub kernels_out: *mut i32,
}

/// `fl_gemv_resid_args`: the decode stream's residual epilogue and the prologue that consumes it (fl_op_gemv_resid, unit tests);
/// `struct_size` is `size_of::<fl_gemv_resid_args>()`.
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct fl_gemv_resid_args {
    pub struct_size: usize,
    pub mode: i32,
    pub epi2: i32,
    pub repeat: i32,
    pub reserved: i32,
    pub n: i64,
    pub k: i64,
    pub n2: i64,
    pub h: i64,
    pub hkv: i64,
    pub d: i64,
    pub max_pos: i64,
    pub pos: i64,
    pub len: i64,
    pub seq_alloc: i64,
    pub x: *const c_void,
    pub w: *const c_void,
    pub h_in: *const f32,
    pub w_next: *const f32,
    pub xs: *const c_void,
    pub cs: *const f32,
    pub w2: *const c_void,
    pub cos_tab: *const f32,
    pub sin_tab: *const f32,
    pub eps: f32,
    pub reserved2: f32,
    pub h_out: *mut f32,
    pub xs_out: *mut c_void,
    pub cs_out: *mut f32,
    pub delta_out: *mut f32,
    pub y_out: *mut f32,
    pub inv_out: *mut f32,
    pub h_ref: *mut f32,
    pub y_ref: *mut f32,
    pub inv_ref: *mut f32,
    pub amax_out: *mut i32,
}

/// `fl_rope_seqs`: the sequences of an fl_op_rope_kv / fl_op_qkv_rope call -- per sequence its new rows, RoPE position, cache length,
/// capacity and value layout, and its whole K / V caches (updated in place).
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct fl_rope_seqs {
    pub n_seq: i32,
    pub layers: i32,
    pub layer: i32,
    pub reserved: i32,
    pub count: *const i32,
    pub pos: *const i32,
    pub len: *const i32,
    pub seq_alloc: *const i32,
    pub v_transposed: *const i32,
    pub k_cache: *const *mut c_void,
    pub v_cache: *const *mut c_void,
}

/// `fl_rope_kv_args`: the stand-alone RoPE + KV-append kernels on host buffers (fl_op_rope_kv, unit tests); `struct_size` is
/// `size_of::<fl_rope_kv_args>()`.
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct fl_rope_kv_args {
    pub struct_size: usize,
    pub form: i32,
    pub dtype: i32,
    pub n_slab: i32,
    pub repeat: i32,
    pub h: i64,
    pub hkv: i64,
    pub d: i64,
    pub max_pos: i64,
    pub qkv: *const f32,
    pub bias: *const f32,
    pub cos_tab: *const f32,
    pub sin_tab: *const f32,
    pub seqs: fl_rope_seqs,
    pub q_out: *mut c_void,
    pub kernels_out: *mut i32,
}

/// `fl_qkv_rope_args`: residual add -> RMSNorm -> QKV projection with the RoPE + KV-append epilogue in a named form (fl_op_qkv_rope,
/// unit tests); `struct_size` is `size_of::<fl_qkv_rope_args>()`.
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct fl_qkv_rope_args {
    pub struct_size: usize,
    pub form: i32,
    pub dtype: i32,
    pub n_slab: i32,
    pub repeat: i32,
    pub t: i64,
    pub k: i64,
    pub h: i64,
    pub hkv: i64,
    pub d: i64,
    pub max_pos: i64,
    pub vocab: i64,
    pub x_res: *const f32,
    pub delta: *const f32,
    pub norm_w: *const f32,
    pub embed: *const c_void,
    pub tokens: *const u32,
    pub w: *const c_void,
    pub w_scale: *const f32,
    pub bias: *const f32,
    pub cos_tab: *const f32,
    pub sin_tab: *const f32,
    pub eps: f32,
    pub reserved: f32,
    pub seqs: fl_rope_seqs,
    pub q_out: *mut c_void,
    pub x_out: *mut f32,
    pub kernels_out: *mut i32,
}

/// `fl_encoder_rows_args`: the encoder's LayerNorm, bias + GELU and pooling kernels alone on host buffers (fl_op_encoder_rows, unit
/// tests); `struct_size` is `size_of::<fl_encoder_rows_args>()`.
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct fl_encoder_rows_args {
    pub struct_size: usize,
    pub form: i32,
    pub dtype: i32,
    pub n_slab: i32,
    pub repeat: i32,
    pub act: i32,
    pub reserved: i32,
    pub t: i64,
    pub h: i64,
    pub vocab: i64,
    pub p: i64,
    pub n_seq: usize,
    pub word: *const c_void,
    pub pos: *const c_void,
    pub tt0: *const c_void,
    pub ids: *const u32,
    pub offsets: *const usize,
    pub x: *const f32,
    pub slabs: *const f32,
    pub bias: *const f32,
    pub ln_w: *const f32,
    pub ln_b: *const f32,
    pub eps: f32,
    pub reserved2: f32,
    pub x_res_out: *mut f32,
    pub out: *mut c_void,
}

/// `fl_convert_slice_args`: the weight conversion launch of the model build alone on host buffers (fl_op_convert_slice, unit tests);
/// `struct_size` is `size_of::<fl_convert_slice_args>()`.
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct fl_convert_slice_args {
    pub struct_size: usize,
    pub src_dtype: i32,
    pub dst_dtype: i32,
    pub row_mode: i32,
    pub head_pad: i32,
    pub via_bf16: i32,
    pub reserved: i32,
    pub r: i64,
    pub c: i64,
    pub r0: i64,
    pub c0: i64,
    pub rows: i64,
    pub cols: i64,
    pub dst_rows: i64,
    pub dst_ld: i64,
    pub dst_row0: i64,
    pub dm: i64,
    pub d: i64,
    pub src: *const c_void,
    pub dst: *mut c_void,
}

// fl_model_tensor_sel: the device tensors fl_op_model_tensor copies out; FL_ELEM_E4M3: the element code of the *_Q tensors
pub const FL_ELEM_E4M3: i32 = 3;
pub const FL_MT_EMBED: i32 = 0;
pub const FL_MT_NORM: i32 = 1;
pub const FL_MT_LM_HEAD: i32 = 2;
pub const FL_MT_COS_TAB: i32 = 3;
pub const FL_MT_SIN_TAB: i32 = 4;
pub const FL_MT_WQKV: i32 = 5;
pub const FL_MT_BQKV: i32 = 6;
pub const FL_MT_WO: i32 = 7;
pub const FL_MT_WGU: i32 = 8;
pub const FL_MT_WD: i32 = 9;
pub const FL_MT_LN1: i32 = 10;
pub const FL_MT_LN2: i32 = 11;
pub const FL_MT_WQKV_Q: i32 = 12;
pub const FL_MT_WQKV_S: i32 = 13;
pub const FL_MT_WO_Q: i32 = 14;
pub const FL_MT_WO_S: i32 = 15;
pub const FL_MT_WGU_Q: i32 = 16;
pub const FL_MT_WGU_S: i32 = 17;
pub const FL_MT_WD_Q: i32 = 18;
pub const FL_MT_WD_S: i32 = 19;
pub const FL_MT_LM_HEAD_Q: i32 = 20;
pub const FL_MT_LM_HEAD_S: i32 = 21;

/// `fl_attn_oproj_rep_args`: decode attention replicated inside the o_proj launch on host buffers (fl_op_attn_oproj_rep, unit tests);
/// `struct_size` is `size_of::<fl_attn_oproj_rep_args>()`.
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct fl_attn_oproj_rep_args {
    pub struct_size: usize,
    pub h: i64,
    pub hkv: i64,
    pub d: i64,
    pub n: i64,
    pub s_past: i64,
    pub k_rows: i64,
    pub capacity: i64,
    pub q: *const c_void,
    pub k: *const c_void,
    pub v: *const c_void,
    pub w_o: *const c_void,
    pub pad_value: f32,
    pub repeat: i32,
    pub query_only: i32,
    pub reserved: i32,
    pub out: *mut f32,
    pub info_out: *mut i32,
}

/// `fl_lookup`: prompt-lookup drafting (fl_lookup_draft, fl_decode_lookup); `struct_size` is `size_of::<fl_lookup>()`.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct fl_lookup {
    pub struct_size: u32,
    pub max_draft: i32,
    pub ngram_max: i32,
    pub ngram_min: i32,
    pub _pad: i32,
    pub _reserved: [i64; 2],
}

/// `fl_spec_stats`: verify steps, drafted ids and accepted ids of one fl_decode_lookup call.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct fl_spec_stats {
    pub steps: u64,
    pub drafted: u64,
    pub accepted: u64,
}

#[repr(C)]
#[derive(Clone, Copy)]
pub struct fl_kernel_stat {
    pub name: [c_char; 48],
    pub launches: i64,
    pub total_ms: f64,
    pub bytes: f64,
    pub flops: f64,
}

/// `fl_encoder_config`: the fields of the reference's BertConfig (src/models/embeddings.rs:46-54) + vocab_size, the GELU form, the
/// HF token-type option and the workspace size.  `struct_size` must be `size_of::<fl_encoder_config>()`; `_reserved` is 0.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct fl_encoder_config {
    pub struct_size: u32,
    pub activation: i32,
    pub add_token_type0: i32,
    pub _pad: i32,
    pub hidden_size: i64,
    pub intermediate_size: i64,
    pub num_hidden_layers: i64,
    pub num_attention_heads: i64,
    pub max_position_embeddings: i64,
    pub vocab_size: i64,
    pub max_batch_tokens: i64,
    pub layer_norm_eps: f64,
    pub _reserved: [i64; 2],
}

/// Opaque handles.
#[repr(C)]
pub struct fl_model {
    _private: [u8; 0],
}
#[repr(C)]
pub struct fl_cache {
    _private: [u8; 0],
}
#[repr(C)]
pub struct fl_batch {
    _private: [u8; 0],
}
#[repr(C)]
pub struct fl_guide {
    _private: [u8; 0],
}
#[repr(C)]
pub struct fl_encoder {
    _private: [u8; 0],
}

extern "C" {
    pub fn fl_abi_version() -> c_int;
    /// Thread-local message of the last failure on this thread; never null.
    pub fn fl_last_error() -> *const c_char;
    pub fn fl_device_count(count: *mut c_int) -> c_int;
    pub fn fl_comm_unique_id(out: *mut c_void) -> c_int;

    pub fn fl_model_create(
        cfg: *const fl_config,
        tensors: *const fl_tensor,
        n_tensors: usize,
        compute_dtype: i32,
        par: *const fl_parallel,
        out: *mut *mut fl_model,
    ) -> c_int;
    pub fn fl_model_create_opts(
        cfg: *const fl_config,
        tensors: *const fl_tensor,
        n_tensors: usize,
        compute_dtype: i32,
        par: *const fl_parallel,
        opts: *const fl_model_options,
        out: *mut *mut fl_model,
    ) -> c_int;
    pub fn fl_comm_ipc_export(m: *mut fl_model, handle_out: *mut c_void) -> c_int;
    pub fn fl_comm_ipc_connect(m: *mut fl_model, handles: *const c_void) -> c_int;
    pub fn fl_model_retain(m: *mut fl_model);
    pub fn fl_model_release(m: *mut fl_model);
    pub fn fl_model_get_info(m: *const fl_model, out: *mut fl_model_info) -> c_int;

    pub fn fl_cache_create(m: *mut fl_model, max_seq: usize, out: *mut *mut fl_cache) -> c_int;
    pub fn fl_cache_reset(c: *mut fl_cache);
    pub fn fl_cache_len(c: *const fl_cache) -> usize;
    pub fn fl_cache_capacity(c: *const fl_cache) -> usize;
    pub fn fl_cache_destroy(c: *mut fl_cache);

    pub fn fl_forward(m: *mut fl_model, c: *mut fl_cache, ids: *const u32, t: usize, pos: usize, logits_out: *mut f32) -> c_int;
    pub fn fl_forward_argmax(m: *mut fl_model, c: *mut fl_cache, ids: *const u32, t: usize, pos: usize, token_out: *mut u32) -> c_int;
    pub fn fl_decode_greedy(
        m: *mut fl_model,
        c: *mut fl_cache,
        first_token: u32,
        pos: usize,
        n_steps: usize,
        eos: i64,
        tokens_out: *mut u32,
        n_out: *mut usize,
    ) -> c_int;
    pub fn fl_forward_sample(
        m: *mut fl_model,
        c: *mut fl_cache,
        ids: *const u32,
        t: usize,
        pos: usize,
        sampling: *const fl_sampling,
        token_out: *mut u32,
    ) -> c_int;
    pub fn fl_decode_sample(
        m: *mut fl_model,
        c: *mut fl_cache,
        first_token: u32,
        pos: usize,
        n_steps: usize,
        eos: i64,
        sampling: *const fl_sampling,
        tokens_out: *mut u32,
        n_out: *mut usize,
    ) -> c_int;
    pub fn fl_forward_sample_ex(
        m: *mut fl_model,
        c: *mut fl_cache,
        ids: *const u32,
        t: usize,
        pos: usize,
        sampler: *const fl_sampler,
        token_out: *mut u32,
    ) -> c_int;
    pub fn fl_decode_sample_ex(
        m: *mut fl_model,
        c: *mut fl_cache,
        first_token: u32,
        pos: usize,
        n_steps: usize,
        eos: i64,
        sampler: *const fl_sampler,
        tokens_out: *mut u32,
        n_out: *mut usize,
    ) -> c_int;

    pub fn fl_cache_truncate(c: *mut fl_cache, len: usize) -> c_int;
    pub fn fl_cache_copy_prefix(dst: *mut fl_cache, src: *const fl_cache, n: usize) -> c_int;
    pub fn fl_forward_verify(
        m: *mut fl_model,
        c: *mut fl_cache,
        token: u32,
        draft: *const u32,
        n_draft: usize,
        pos: usize,
        tokens_out: *mut u32,
        n_out: *mut usize,
        logits_out: *mut f32,
    ) -> c_int;
    pub fn fl_lookup_draft(
        history: *const u32,
        n_history: usize,
        opts: *const fl_lookup,
        limit: usize,
        draft_out: *mut u32,
        n_draft_out: *mut usize,
    ) -> c_int;
    pub fn fl_decode_lookup(
        m: *mut fl_model,
        c: *mut fl_cache,
        corpus: *const u32,
        n_corpus: usize,
        first_token: u32,
        pos: usize,
        n_steps: usize,
        eos: i64,
        opts: *const fl_lookup,
        tokens_out: *mut u32,
        n_out: *mut usize,
        stats: *mut fl_spec_stats,
    ) -> c_int;
    pub fn fl_forward_verify_ex(
        m: *mut fl_model,
        c: *mut fl_cache,
        token: u32,
        draft: *const u32,
        n_draft: usize,
        pos: usize,
        sampler: *const fl_sampler,
        tokens_out: *mut u32,
        n_out: *mut usize,
        logits_out: *mut f32,
    ) -> c_int;
    pub fn fl_decode_lookup_ex(
        m: *mut fl_model,
        c: *mut fl_cache,
        corpus: *const u32,
        n_corpus: usize,
        first_token: u32,
        pos: usize,
        n_steps: usize,
        eos: i64,
        opts: *const fl_lookup,
        sampler: *const fl_sampler,
        tokens_out: *mut u32,
        n_out: *mut usize,
        stats: *mut fl_spec_stats,
    ) -> c_int;
    /// The same two calls on a cache that may have logit rules and / or a guide, with optional log-probs (`lp` null: none).
    pub fn fl_forward_verify_lp(
        m: *mut fl_model,
        c: *mut fl_cache,
        token: u32,
        draft: *const u32,
        n_draft: usize,
        pos: usize,
        sampler: *const fl_sampler,
        lp: *const fl_logprobs,
        tokens_out: *mut u32,
        n_out: *mut usize,
        logits_out: *mut f32,
    ) -> c_int;
    pub fn fl_decode_lookup_lp(
        m: *mut fl_model,
        c: *mut fl_cache,
        corpus: *const u32,
        n_corpus: usize,
        first_token: u32,
        pos: usize,
        n_steps: usize,
        eos: i64,
        opts: *const fl_lookup,
        sampler: *const fl_sampler,
        lp: *const fl_logprobs,
        tokens_out: *mut u32,
        n_out: *mut usize,
        stats: *mut fl_spec_stats,
    ) -> c_int;
    /// The verify steps of up to 64 streams as the rows of one packed forward, and the lookup loop built from such steps.
    pub fn fl_batch_verify(
        m: *mut fl_model,
        caches: *const *mut fl_cache,
        n: usize,
        ids: *const u32,
        offsets: *const usize,
        pos: *const usize,
        samplers: *const fl_sampler,
        tokens_out: *mut u32,
        n_out: *mut usize,
        logits_out: *mut f32,
    ) -> c_int;
    pub fn fl_batch_decode_lookup(
        m: *mut fl_model,
        caches: *const *mut fl_cache,
        n: usize,
        corpus: *const u32,
        corpus_offsets: *const usize,
        first_tokens: *const u32,
        pos: *const usize,
        n_steps: *const usize,
        eos: *const i64,
        opts: *const fl_lookup,
        samplers: *const fl_sampler,
        tokens_out: *mut u32,
        n_out: *mut usize,
        stats: *mut fl_spec_stats,
    ) -> c_int;
    pub fn fl_op_verify_packed(
        logits: *const f32,
        t: i64,
        v: i64,
        n_seq: usize,
        offsets: *const usize,
        ids: *const u32,
        samplers: *const fl_sampler,
        block_rows: i64,
        tokens_out: *mut u32,
        n_acc_out: *mut i64,
        kept_out: *mut i64,
        iters: i32,
        ms_out: *mut f64,
    ) -> c_int;

    pub fn fl_batch_create(m: *mut fl_model, caches: *const *mut fl_cache, n: usize, out: *mut *mut fl_batch) -> c_int;
    pub fn fl_batch_destroy(b: *mut fl_batch);
    pub fn fl_batch_replace(b: *mut fl_batch, slot: usize, cache: *mut fl_cache) -> c_int;
    pub fn fl_batch_forward(b: *mut fl_batch, tokens: *const u32, pos: *const usize, logits_out: *mut f32, argmax_out: *mut u32) -> c_int;
    pub fn fl_batch_prefill(
        m: *mut fl_model,
        caches: *const *mut fl_cache,
        n: usize,
        ids: *const u32,
        offsets: *const usize,
        pos: *const usize,
        samplers: *const fl_sampler,
        tokens_out: *mut u32,
        logits_out: *mut f32,
    ) -> c_int;
    pub fn fl_batch_decode(
        b: *mut fl_batch,
        first_tokens: *const u32,
        pos: *const usize,
        n_steps: usize,
        eos: i64,
        sampling: *const fl_sampling,
        tokens_out: *mut u32,
        n_out: *mut usize,
    ) -> c_int;
    pub fn fl_batch_decode_each(
        b: *mut fl_batch,
        first_tokens: *const u32,
        pos: *const usize,
        n_steps: usize,
        eos: *const i64,
        sampling: *const fl_sampling,
        tokens_out: *mut u32,
        n_out: *mut usize,
    ) -> c_int;
    pub fn fl_batch_decode_each_ex(
        b: *mut fl_batch,
        first_tokens: *const u32,
        pos: *const usize,
        n_steps: usize,
        eos: *const i64,
        samplers: *const fl_sampler,
        tokens_out: *mut u32,
        n_out: *mut usize,
    ) -> c_int;

    /// The sampled entry points with log-probabilities (`sampler` null: ArgMax); tokens, cache state and draw count are those of the
    /// `_ex` calls.
    pub fn fl_forward_sample_lp(
        m: *mut fl_model,
        c: *mut fl_cache,
        ids: *const u32,
        t: usize,
        pos: usize,
        sampler: *const fl_sampler,
        token_out: *mut u32,
        lp: *const fl_logprobs,
    ) -> c_int;
    pub fn fl_decode_sample_lp(
        m: *mut fl_model,
        c: *mut fl_cache,
        first_token: u32,
        pos: usize,
        n_steps: usize,
        eos: i64,
        sampler: *const fl_sampler,
        tokens_out: *mut u32,
        n_out: *mut usize,
        lp: *const fl_logprobs,
    ) -> c_int;
    pub fn fl_batch_decode_each_lp(
        b: *mut fl_batch,
        first_tokens: *const u32,
        pos: *const usize,
        n_steps: usize,
        eos: *const i64,
        samplers: *const fl_sampler,
        tokens_out: *mut u32,
        n_out: *mut usize,
        lp: *const fl_logprobs,
    ) -> c_int;
    pub fn fl_op_logprobs(
        logits: *const f32,
        t: i64,
        v: i64,
        chosen: *const u32,
        top_n: i32,
        token_logprob: *mut f32,
        top_ids: *mut u32,
        top_logprobs: *mut f32,
    ) -> c_int;
    /// `fl_forward` / `fl_batch_prefill` with every row scored on the device (prompt log-probabilities); nothing is selected.
    pub fn fl_forward_score(m: *mut fl_model, c: *mut fl_cache, ids: *const u32, t: usize, pos: usize, sc: *const fl_score) -> c_int;
    pub fn fl_batch_score(
        m: *mut fl_model,
        caches: *const *mut fl_cache,
        n: usize,
        ids: *const u32,
        offsets: *const usize,
        pos: *const usize,
        sc: *const fl_score,
    ) -> c_int;
    /// `fl_batch_prefill`'s pack with the pooled final hidden states coming back instead of logits (decoder-model embeddings):
    /// `out` is `[n][dims]`, or `[offsets[n]][dims]` with `FL_POOL_NONE`.
    pub fn fl_batch_embed(
        m: *mut fl_model,
        caches: *const *mut fl_cache,
        n: usize,
        ids: *const u32,
        offsets: *const usize,
        pos: *const usize,
        opts: *const fl_embed,
        out: *mut f32,
    ) -> c_int;
    pub fn fl_op_pool_rows(
        x: *const f32,
        inv_rms: *const f32,
        w: *const f32,
        offsets: *const usize,
        n_seq: usize,
        h: i64,
        opts: *const fl_embed,
        out: *mut f32,
    ) -> c_int;
    pub fn fl_op_pool_rows_time(
        x: *const f32,
        inv_rms: *const f32,
        w: *const f32,
        offsets: *const usize,
        n_seq: usize,
        h: i64,
        opts: *const fl_embed,
        iters: i32,
        ms_out: *mut f64,
    ) -> c_int;
    pub fn fl_op_score(
        logits: *const f32,
        t: i64,
        v: i64,
        targets: *const u32,
        top_n: i32,
        target_logprob: *mut f32,
        target_rank: *mut u32,
        top_ids: *mut u32,
        top_logprobs: *mut f32,
    ) -> c_int;
    pub fn fl_op_score_time(logits: *const f32, t: i64, v: i64, targets: *const u32, top_n: i32, iters: i32, ms_out: *mut f64) -> c_int;
    pub fn fl_cache_set_logit_rules(
        m: *mut fl_model,
        c: *mut fl_cache,
        rules: *const fl_logit_rules,
        prompt_ids: *const u32,
        n_prompt: usize,
        output_ids: *const u32,
        n_output: usize,
    ) -> c_int;
    pub fn fl_cache_logit_counts(m: *mut fl_model, c: *mut fl_cache, words_out: *mut u32) -> c_int;
    pub fn fl_op_logit_rules(
        logits: *const f32,
        b: i64,
        v: i64,
        words: *mut u32,
        biases: *const f32,
        scalars: *const f32,
        tokens: *const u32,
        count_input: i32,
        has_rules: *const u8,
        out: *mut f32,
    ) -> c_int;
    pub fn fl_guide_create(m: *mut fl_model, desc: *const fl_guide_desc, out: *mut *mut fl_guide) -> c_int;
    pub fn fl_guide_destroy(g: *mut fl_guide);
    pub fn fl_cache_set_guide(m: *mut fl_model, c: *mut fl_cache, g: *mut fl_guide, state: u32) -> c_int;
    pub fn fl_cache_guide_state(c: *const fl_cache, state_out: *mut u32) -> c_int;
    pub fn fl_op_guide_mask(
        logits: *const f32,
        b: i64,
        v: i64,
        desc: *const fl_guide_desc,
        states: *const u32,
        tokens: *const u32,
        has_guide: *const u8,
        out: *mut f32,
        next_states: *mut u32,
    ) -> c_int;
    pub fn fl_op_verify_adjust(
        logits: *const f32,
        t: i64,
        v: i64,
        ids: *const u32,
        words: *mut u32,
        biases: *const f32,
        scalars: *const f32,
        desc: *const fl_guide_desc,
        states: *const u32,
        out: *mut f32,
    ) -> c_int;
    pub fn fl_op_verify_adjust_time(
        logits: *const f32,
        t: i64,
        v: i64,
        ids: *const u32,
        words: *const u32,
        biases: *const f32,
        scalars: *const f32,
        desc: *const fl_guide_desc,
        states: *const u32,
        iters: i32,
        ms_out: *mut f64,
    ) -> c_int;
    pub fn fl_op_rules_count(words: *mut u32, v: i64, ids: *const u32, n: i64) -> c_int;

    pub fn fl_synchronize(m: *mut fl_model) -> c_int;

    /// The BERT / MiniLM encoder (the reference's EmbeddingModel path, src/models/embeddings.rs) on GPU `device`.
    pub fn fl_encoder_create(
        cfg: *const fl_encoder_config,
        tensors: *const fl_tensor,
        n_tensors: usize,
        compute_dtype: i32,
        device: i32,
        out: *mut *mut fl_encoder,
    ) -> c_int;
    pub fn fl_encoder_release(e: *mut fl_encoder);
    /// Last hidden states of one sequence, `[t][hidden_size]` f32.
    pub fn fl_encoder_hidden(e: *mut fl_encoder, ids: *const u32, t: usize, out: *mut f32) -> c_int;
    /// `n_seq` packed sequences (`offsets[n_seq + 1]`) -> `[n_seq][hidden_size]` L2-normalised mean-pooled embeddings.
    pub fn fl_encoder_embed(e: *mut fl_encoder, ids: *const u32, offsets: *const usize, n_seq: usize, out: *mut f32) -> c_int;
    pub fn fl_op_encoder_attention(
        q: *const c_void,
        k: *const c_void,
        v: *const c_void,
        offsets: *const usize,
        n_seq: usize,
        h: i64,
        d: i64,
        dtype: i32,
        out: *mut f32,
    ) -> c_int;
    pub fn fl_tp_slice(cfg: *const fl_config, tensor_name: *const c_char, tp_rank: i32, tp_size: i32, out: *mut i64) -> c_int;

    pub fn fl_profile_begin(m: *mut fl_model) -> c_int;
    pub fn fl_profile_end(m: *mut fl_model, stats: *mut fl_kernel_stat, cap: usize, n_stats: *mut usize) -> c_int;
    pub fn fl_comm_probe(m: *mut fl_model, form: i32, n: i64, iters: i32, us_per_call: *mut f64) -> c_int;
    pub fn fl_comm_selftest(m: *mut fl_model, n: i64, ok: *mut i32) -> c_int;
    pub fn fl_tune(key: *const c_char, value: c_int) -> c_int;
    pub fn fl_op_linear(
        x: *const c_void,
        w: *const c_void,
        bias: *const f32,
        t: i64,
        n: i64,
        k: i64,
        dtype: i32,
        epilogue: i32,
        y: *mut f32,
        iters: i32,
        ms_out: *mut f64,
    ) -> c_int;
    pub fn fl_op_quantize_rows(w: *const c_void, dtype: i32, n: i64, k: i64, q_out: *mut u8, s_out: *mut f32) -> c_int;
    pub fn fl_op_gemv_w8(
        x: *const c_void,
        q: *const u8,
        s: *const f32,
        bias: *const f32,
        n: i64,
        k: i64,
        epilogue: i32,
        y: *mut f32,
        iters: i32,
        ms_out: *mut f64,
    ) -> c_int;
    pub fn fl_op_rmsnorm_add(
        x_res: *mut f32,
        delta: *const f32,
        n_slab: i32,
        w: *const f32,
        eps: f32,
        t: i64,
        h: i64,
        dtype: i32,
        xs_out: *mut f32,
        inv_rms_out: *mut f32,
    ) -> c_int;
    pub fn fl_op_norm_linear(args: *const fl_norm_linear_args) -> c_int;
    pub fn fl_op_linear_resid(args: *const fl_linear_resid_args) -> c_int;
    pub fn fl_op_gemv_resid(args: *const fl_gemv_resid_args) -> c_int;
    pub fn fl_op_rope_kv(args: *const fl_rope_kv_args) -> c_int;
    pub fn fl_op_qkv_rope(args: *const fl_qkv_rope_args) -> c_int;
    pub fn fl_op_attn_oproj_rep(args: *const fl_attn_oproj_rep_args) -> c_int;
    pub fn fl_op_encoder_rows(args: *const fl_encoder_rows_args) -> c_int;
    pub fn fl_op_convert_slice(args: *const fl_convert_slice_args) -> c_int;
    pub fn fl_op_model_tensor(
        m: *mut fl_model,
        shard: i32,
        selector: i32,
        layer: i64,
        out: *mut c_void,
        rows_out: *mut i64,
        cols_out: *mut i64,
        elem_out: *mut i32,
    ) -> c_int;
    pub fn fl_op_sample(logits: *const f32, v: i64, sampling: *const fl_sampling, n_draws: i64, tokens_out: *mut u32) -> c_int;
    pub fn fl_op_sample_ex(logits: *const f32, v: i64, sampler: *const fl_sampler, n_draws: i64, tokens_out: *mut u32, kept_out: *mut i64) -> c_int;
    pub fn fl_op_verify_select(logits: *const f32, t: i64, v: i64, draft: *const u32, argmax_out: *mut u32, n_accepted_out: *mut i64) -> c_int;
    pub fn fl_op_verify_sample(
        logits: *const f32,
        t: i64,
        v: i64,
        draft: *const u32,
        sampler: *const fl_sampler,
        tokens_out: *mut u32,
        n_accepted_out: *mut i64,
        kept_out: *mut i64,
    ) -> c_int;
    pub fn fl_op_verify_sample_time(logits: *const f32, t: i64, v: i64, sampler: *const fl_sampler, iters: *const i32, ms_out: *mut f64) -> c_int;
    pub fn fl_op_kv_copy(
        src: *const c_void,
        dst: *mut c_void,
        rows: i64,
        width_bytes: i64,
        src_pitch: i64,
        dst_pitch: i64,
        iters: i32,
        ms_out: *mut f64,
    ) -> c_int;
    pub fn fl_op_attention(
        q: *const c_void,
        k: *const c_void,
        v: *const c_void,
        t: i64,
        s_past: i64,
        h: i64,
        hkv: i64,
        d: i64,
        window: i64,
        kernel: i32,
        nsplit: i32,
        out: *mut f32,
    ) -> c_int;
    pub fn fl_op_attention_plain(
        q: *const c_void,
        k: *const c_void,
        v: *const c_void,
        dtype: i32,
        layout: i32,
        kernel: i32,
        t: i64,
        s_past: i64,
        call0: i64,
        k_rows: i64,
        capacity: i64,
        h: i64,
        hkv: i64,
        d: i64,
        window: i64,
        nsplit: i32,
        pad_value: f32,
        repeat: i32,
        out: *mut f32,
    ) -> c_int;
    pub fn fl_op_attention_batch(
        q: *const c_void,
        k: *const *const c_void,
        v: *const *const c_void,
        dtype: i32,
        layout: i32,
        b: i64,
        lens: *const i64,
        k_rows: *const i64,
        seq_alloc: *const i64,
        nsplit: *const i32,
        n_layers: i64,
        layer: i64,
        h: i64,
        hkv: i64,
        d: i64,
        pad_value: f32,
        repeat: i32,
        out: *mut f32,
    ) -> c_int;
    pub fn fl_op_attention_packed(
        q: *const c_void,
        k: *const *const c_void,
        v: *const *const c_void,
        n_seq: i64,
        offsets: *const i64,
        s_past: *const i64,
        k_rows: *const i64,
        seq_alloc: *const i64,
        n_layers: i64,
        layer: i64,
        h: i64,
        hkv: i64,
        d: i64,
        window: i64,
        pad_value: f32,
        out: *mut f32,
    ) -> c_int;
    pub fn fl_op_attention_packed_ex(
        q: *const c_void,
        k: *const *const c_void,
        v: *const *const c_void,
        n_seq: i64,
        offsets: *const i64,
        s_past: *const i64,
        k_rows: *const i64,
        seq_alloc: *const i64,
        n_layers: i64,
        layer: i64,
        h: i64,
        hkv: i64,
        d: i64,
        window: i64,
        pad_value: f32,
        mask: i32,
        out: *mut f32,
    ) -> c_int;
}
