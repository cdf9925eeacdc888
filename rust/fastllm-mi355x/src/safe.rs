//! Safe layer over [`crate::ffi`]: RAII handles and `Result`s.  No candle types here -- tensors come in as
//! [`TensorView`]s (name, dtype, shape, bytes) and logits go out as `Vec<f32>`; the trait glue that converts candle's
//! `Tensor` to and from these lives in the patched reference tree (`src/models/mi355x.rs`).
use std::ffi::{CStr, CString};
use std::fmt;
use std::os::raw::c_void;
use std::ptr;

use crate::ffi;

/// A failed library call: the status code and `fl_last_error()` of the calling thread.
#[derive(Debug, Clone)]
pub struct Error {
    pub code: i32,
    pub message: String,
}
impl fmt::Display for Error {
    fn fmt(&self, f: &mut fmt::Formatter<'_>) -> fmt::Result {
        write!(f, "fastllm_mi355x error {}: {}", self.code, self.message)
    }
}
impl std::error::Error for Error {}
pub type Result<T> = std::result::Result<T, Error>;

fn check(rc: i32) -> Result<()> {
    if rc == ffi::FL_OK {
        return Ok(());
    }
    // SAFETY: fl_last_error never returns null and the buffer is thread-local to this thread.
    let message = unsafe { CStr::from_ptr(ffi::fl_last_error()) }.to_string_lossy().into_owned();
    Err(Error { code: rc, message })
}

#[derive(Clone, Copy, Debug, PartialEq, Eq)]
#[repr(i32)]
pub enum Family {
    Llama = ffi::FL_FAMILY_LLAMA,
    Mistral = ffi::FL_FAMILY_MISTRAL,
    Qwen2 = ffi::FL_FAMILY_QWEN2,
}

#[derive(Clone, Copy, Debug, PartialEq, Eq)]
#[repr(i32)]
pub enum DType {
    F32 = ffi::FL_DTYPE_F32,
    BF16 = ffi::FL_DTYPE_BF16,
    F16 = ffi::FL_DTYPE_F16,
}

/// The fields of the reference's `BaseModelConfig` (src/models/config.rs:6-18); `None` = absent from config.json, the
/// library applies the reference's default (llama.rs:39-47, mistral.rs:97-139, qwen.rs:45-49).
#[derive(Clone, Debug)]
pub struct Config {
    pub family: Family,
    pub hidden_size: usize,
    pub intermediate_size: usize,
    pub vocab_size: usize,
    pub num_hidden_layers: usize,
    pub num_attention_heads: usize,
    pub num_key_value_heads: Option<usize>,
    pub rms_norm_eps: f64,
    pub rope_theta: Option<f64>,
    pub max_position_embeddings: Option<usize>,
    pub sliding_window: Option<usize>,
}

impl Config {
    pub fn to_ffi(&self) -> ffi::fl_config {
        ffi::fl_config {
            family: self.family as i32,
            qkv_bias: (self.family == Family::Qwen2) as i32, // q/k/v_proj.bias tensors (qwen.rs:93-117)
            hidden_size: self.hidden_size as i64,
            intermediate_size: self.intermediate_size as i64,
            vocab_size: self.vocab_size as i64,
            num_hidden_layers: self.num_hidden_layers as i64,
            num_attention_heads: self.num_attention_heads as i64,
            num_key_value_heads: self.num_key_value_heads.unwrap_or(0) as i64,
            max_position_embeddings: self.max_position_embeddings.unwrap_or(0) as i64,
            sliding_window: self.sliding_window.unwrap_or(0) as i64,
            rms_norm_eps: self.rms_norm_eps,
            rope_theta: self.rope_theta.unwrap_or(0.0),
        }
    }
}

/// One named tensor handed to [`Model::new`]: host bytes (`device < 0`) or a device pointer on HIP device `device`.
/// Borrowed for the duration of the call only.
pub struct TensorView<'a> {
    pub name: &'a str,
    pub dtype: DType,
    pub shape: &'a [usize],
    pub data: *const c_void,
    pub device: i32,
}

impl<'a> TensorView<'a> {
    pub fn host(name: &'a str, dtype: DType, shape: &'a [usize], bytes: &'a [u8]) -> Self {
        TensorView { name, dtype, shape, data: bytes.as_ptr() as *const c_void, device: -1 }
    }
}

/// LogitsProcessor::new(seed, Some(temperature), None) (mod.rs:373-374); `draws_done` = u32 words of the seeded stream
/// already consumed by this request.
#[derive(Clone, Copy, Debug)]
pub struct Sampling {
    pub temperature: f64,
    pub seed: u64,
    pub draws_done: u64,
}
impl Sampling {
    fn to_ffi(self) -> ffi::fl_sampling {
        ffi::fl_sampling { temperature: self.temperature, seed: self.seed, draws_done: self.draws_done }
    }
}

/// What `Model::decode_sample_logprobs` returns: the emitted tokens, each one's log-probability, and row-major `[n][top_n]` ids and
/// log-probabilities of the most likely tokens of every step.
#[derive(Clone, Debug, Default)]
pub struct TokenLogprobs {
    pub tokens: Vec<u32>,
    pub token_logprob: Vec<f32>,
    pub top_ids: Vec<u32>,
    pub top_logprobs: Vec<f32>,
    pub top_n: usize,
}

/// What `Model::forward_score` returns, one entry per row of the call: the target's log-probability (NaN: the row has none), its
/// rank in the order "logit descending, lower index first" (0: none), and row-major `[T][top_n]` ids and log-probabilities.
#[derive(Clone, Debug, Default)]
pub struct ScoredTokens {
    pub target_logprob: Vec<f32>,
    pub target_rank: Vec<u32>,
    pub top_ids: Vec<u32>,
    pub top_logprobs: Vec<f32>,
    pub top_n: usize,
}

/// LogitsProcessor::from_sampling(seed, Sampling::TopP / TopK / TopKThenTopP) on the device (`fl_sampler`).  `top_p` outside
/// (0, 1) and `top_k` 0 are "off"; both off is `Sampling::All`.  The kept set is a prefix of the order by probability
/// descending, the lower index first among equals; `top_k = 1` therefore keeps the LOWEST maximal index while ArgMax
/// (`temperature < 1e-7`) keeps the LAST.
#[derive(Clone, Copy, Debug)]
pub struct Sampler {
    pub temperature: f64,
    pub top_p: f64,
    pub top_k: u32,
    pub seed: u64,
    pub draws_done: u64,
}
impl Sampler {
    fn to_ffi(self) -> ffi::fl_sampler {
        ffi::fl_sampler {
            struct_size: std::mem::size_of::<ffi::fl_sampler>() as u32,
            top_k: self.top_k.min(i32::MAX as u32) as i32,
            temperature: self.temperature,
            top_p: self.top_p,
            seed: self.seed,
            draws_done: self.draws_done,
            _reserved: [0; 2],
        }
    }
}

/// `fl_logit_rules`: an OpenAI-style request's `logit_bias` (id, bias) pairs -- ids distinct, `f32::NEG_INFINITY` bans one -- and its
/// penalties.  `repetition_penalty` 1 and the other two 0 are off.  Installed on a cache with [`Cache::set_logit_rules`].
#[derive(Clone, Debug)]
pub struct LogitRules {
    pub logit_bias: Vec<(u32, f32)>,
    pub repetition_penalty: f32,
    pub frequency_penalty: f32,
    pub presence_penalty: f32,
}
impl Default for LogitRules {
    fn default() -> Self {
        LogitRules { logit_bias: Vec::new(), repetition_penalty: 1.0, frequency_penalty: 0.0, presence_penalty: 0.0 }
    }
}

/// `fl_guide`: an immutable token-level automaton of one model -- what a grammar, JSON-schema or regex compiler emits as an index
/// over token ids.  State `s` allows `tokens[row_ptr[s] .. row_ptr[s + 1]]` (strictly ascending), and `tokens[e]` leads to state
/// `next[e]`.  Shareable by any number of the model's caches ([`Cache::set_guide`]); a cache that has it installed keeps it alive.
pub struct Guide {
    raw: *mut ffi::fl_guide,
    n_states: u32,
}
// SAFETY: immutable after creation and reference-counted inside the library
unsafe impl Send for Guide {}
unsafe impl Sync for Guide {}
impl Drop for Guide {
    fn drop(&mut self) {
        unsafe { ffi::fl_guide_destroy(self.raw) };
    }
}
impl Guide {
    /// `fl_guide_create`.  Errors (`FL_ERR_BAD_ARGUMENT`, before the device is probed): a state without an edge, a list that is not
    /// strictly ascending, an id beyond the vocabulary, a `next` beyond the states, a `row_ptr` that does not start at 0 or decreases;
    /// `FL_ERR_UNSUPPORTED`: a tensor-parallel model.
    pub fn new(model: &Model, row_ptr: &[u64], tokens: &[u32], next: &[u32]) -> Result<Guide> {
        if row_ptr.is_empty() || tokens.len() != next.len() || row_ptr[row_ptr.len() - 1] != tokens.len() as u64 {
            return Err(Error { code: ffi::FL_ERR_BAD_ARGUMENT, message: "guide: row_ptr, tokens and next do not describe one CSR".to_string() });
        }
        let d = ffi::fl_guide_desc {
            struct_size: std::mem::size_of::<ffi::fl_guide_desc>() as u32,
            n_states: (row_ptr.len() - 1) as u32,
            row_ptr: row_ptr.as_ptr(),
            tokens: tokens.as_ptr(),
            next: next.as_ptr(),
            _reserved: [0; 2],
        };
        let mut raw = ptr::null_mut();
        check(unsafe { ffi::fl_guide_create(model.raw, &d, &mut raw) })?;
        Ok(Guide { raw, n_states: d.n_states })
    }
    pub fn n_states(&self) -> u32 {
        self.n_states
    }
}

/// The token-selection kernel alone (`fl_op_sample_ex`): `n_draws` successive draws from one logits vector; returns the
/// tokens and how many tokens each draw kept.
pub fn op_sample(logits: &[f32], s: Sampler, n_draws: usize) -> Result<(Vec<u32>, Vec<i64>)> {
    let mut toks = vec![0u32; n_draws];
    let mut kept = vec![0i64; n_draws];
    let sp = s.to_ffi();
    check(unsafe { ffi::fl_op_sample_ex(logits.as_ptr(), logits.len() as i64, &sp, n_draws as i64, toks.as_mut_ptr(), kept.as_mut_ptr()) })?;
    Ok((toks, kept))
}

/// Prompt-lookup drafting (`fl_lookup`): the continuation that followed the most recent earlier occurrence of the current n-gram.
/// `max_draft` 0 .. `ffi::FL_VERIFY_MAX_DRAFT` (0: plain greedy steps); 1 <= `ngram_min` <= `ngram_max` <= 8.
#[derive(Clone, Copy, Debug)]
pub struct Lookup {
    pub max_draft: u32,
    pub ngram_max: u32,
    pub ngram_min: u32,
}
impl Default for Lookup {
    fn default() -> Self {
        Lookup { max_draft: 7, ngram_max: 3, ngram_min: 1 }
    }
}
impl Lookup {
    fn to_ffi(self) -> ffi::fl_lookup {
        ffi::fl_lookup {
            struct_size: std::mem::size_of::<ffi::fl_lookup>() as u32,
            max_draft: self.max_draft.min(i32::MAX as u32) as i32,
            ngram_max: self.ngram_max.min(i32::MAX as u32) as i32,
            ngram_min: self.ngram_min.min(i32::MAX as u32) as i32,
            _pad: 0,
            _reserved: [0; 2],
        }
    }
}

/// `fl_lookup_draft` (pure host): the draft for `history`, at most `min(max_draft, limit)` ids.
pub fn lookup_draft(history: &[u32], opts: Lookup, limit: usize) -> Result<Vec<u32>> {
    let mut out = vec![0u32; limit.max(1)];
    let mut n = 0usize;
    let o = opts.to_ffi();
    check(unsafe { ffi::fl_lookup_draft(history.as_ptr(), history.len(), &o, limit, out.as_mut_ptr(), &mut n) })?;
    out.truncate(n);
    Ok(out)
}

/// The verify step's selection kernel alone (`fl_op_verify_select`): `logits` is `[draft.len() + 1][v]`; returns the ArgMax of every
/// row and how many drafted ids the rows confirm.
pub fn op_verify_select(logits: &[f32], v: usize, draft: &[u32]) -> Result<(Vec<u32>, usize)> {
    let t = draft.len() + 1;
    if v == 0 || logits.len() != t * v {
        return Err(Error { code: ffi::FL_ERR_BAD_ARGUMENT, message: format!("logits must hold {} rows of {} values", t, v) });
    }
    let mut am = vec![0u32; t];
    let mut n = 0i64;
    check(unsafe { ffi::fl_op_verify_select(logits.as_ptr(), t as i64, v as i64, draft.as_ptr(), am.as_mut_ptr(), &mut n) })?;
    Ok((am, n as usize))
}

/// `fl_pooling`: which rows of a member `Model::embed_packed` returns.
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
#[repr(i32)]
pub enum Pooling {
    Last = ffi::FL_POOL_LAST,
    Mean = ffi::FL_POOL_MEAN,
    First = ffi::FL_POOL_FIRST,
    None = ffi::FL_POOL_NONE,
}

/// `fl_attn_mask`.
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
#[repr(i32)]
pub enum Mask {
    Causal = ffi::FL_MASK_CAUSAL,
    Full = ffi::FL_MASK_FULL,
}

/// The options of `Model::embed_packed` (`fl_embed`).  e5-mistral / SFR / Linq: `Last` + `Causal`; gte-Qwen2: `Last` + `Full`;
/// LLM2Vec Llama: `Mean` + `Full`; reward / classification heads: `None`, unnormalised.
#[derive(Clone, Copy, Debug)]
pub struct EmbedOptions {
    pub pooling: Pooling,
    pub mask: Mask,
    pub normalize: bool,
    pub dimensions: usize,
}

/// `fl_weight_format`: what the single-stream decode step reads its projection weights as.
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
#[repr(i32)]
pub enum WeightFormat {
    ComputeDtype = ffi::FL_WEIGHTS_COMPUTE_DTYPE,
    E4m3Row = ffi::FL_WEIGHTS_E4M3_ROW,
}

/// `fl_model*`.  Immutable after creation; `Clone` is a reference-count bump (the streaming path clones the model per
/// request, mod.rs:155,181,207).
pub struct Model {
    raw: *mut ffi::fl_model,
    vocab: usize,
}
// SAFETY: the library serialises submission per model and every entry sets its HIP device itself
// (include/fastllm_mi355x.h, "thread-safe: any number of threads ... with DISTINCT caches").
unsafe impl Send for Model {}
unsafe impl Sync for Model {}

impl Clone for Model {
    fn clone(&self) -> Self {
        unsafe { ffi::fl_model_retain(self.raw) };
        Model { raw: self.raw, vocab: self.vocab }
    }
}
impl Drop for Model {
    fn drop(&mut self) {
        unsafe { ffi::fl_model_release(self.raw) };
    }
}

impl Model {
    /// `ModelInitializer::initialize_model` (model_initializer.rs:10-17): single GPU `device_id`.
    pub fn new(cfg: &Config, tensors: &[TensorView<'_>], compute: DType, device_id: i32) -> Result<Model> {
        Model::new_with_weights(cfg, tensors, compute, device_id, WeightFormat::ComputeDtype)
    }

    /// ... with the weight format of the decode step (`fl_model_create_opts`).  `WeightFormat::E4m3Row`: bf16 compute only; weight
    /// memory is 1.5x a bf16 model's (the e4m3 bytes and their bf16 image are both kept).
    pub fn new_with_weights(cfg: &Config, tensors: &[TensorView<'_>], compute: DType, device_id: i32, weights: WeightFormat) -> Result<Model> {
        let names: Vec<CString> = tensors
            .iter()
            .map(|t| CString::new(t.name).map_err(|_| Error { code: ffi::FL_ERR_BAD_ARGUMENT, message: format!("tensor name {:?} contains NUL", t.name) }))
            .collect::<Result<_>>()?;
        let mut descr = Vec::with_capacity(tensors.len());
        for (t, name) in tensors.iter().zip(&names) {
            if t.shape.len() > 4 {
                return Err(Error { code: ffi::FL_ERR_SHAPE_MISMATCH, message: format!("tensor {} has rank {}", t.name, t.shape.len()) });
            }
            let mut shape = [0i64; 4];
            for (d, s) in shape.iter_mut().zip(t.shape) {
                *d = *s as i64;
            }
            descr.push(ffi::fl_tensor { name: name.as_ptr(), dtype: t.dtype as i32, ndim: t.shape.len() as i32, shape, data: t.data, device: t.device, _pad: 0 });
        }
        let c = cfg.to_ffi();
        let ids = [device_id];
        let par = ffi::fl_parallel { mode: ffi::FL_TP_NONE, tp_size: 1, tp_rank: 0, n_device_ids: 1, device_ids: ids.as_ptr(), unique_id: ptr::null() };
        let mut raw: *mut ffi::fl_model = ptr::null_mut();
        // SAFETY: every pointer is valid for the duration of the call; the library copies what it keeps.
        let opts = ffi::fl_model_options { struct_size: std::mem::size_of::<ffi::fl_model_options>() as u32, decode_weights: weights as i32, _reserved: [0; 3] };
        check(unsafe { ffi::fl_model_create_opts(&c, descr.as_ptr(), descr.len(), compute as i32, &par, &opts, &mut raw) })?;
        Ok(Model { raw, vocab: cfg.vocab_size })
    }

    pub fn vocab_size(&self) -> usize {
        self.vocab
    }

    pub fn info(&self) -> Result<ffi::fl_model_info> {
        let mut out = ffi::fl_model_info::default();
        check(unsafe { ffi::fl_model_get_info(self.raw, &mut out) })?;
        Ok(out)
    }

    /// `ModelInitializer::initialize_cache` (model_initializer.rs:19; per request, mod.rs:370): caller-owned KV cache.
    pub fn new_cache(&self, max_seq: usize) -> Result<Cache> {
        let mut raw: *mut ffi::fl_cache = ptr::null_mut();
        check(unsafe { ffi::fl_cache_create(self.raw, max_seq, &mut raw) })?;
        Ok(Cache { raw })
    }

    /// `ModelInitializer::forward` (model_initializer.rs:21): last-position logits, `[vocab]` f32.
    pub fn forward(&self, cache: &mut Cache, ids: &[u32], pos: usize) -> Result<Vec<f32>> {
        let mut logits = vec![0f32; self.vocab];
        check(unsafe { ffi::fl_forward(self.raw, cache.raw, ids.as_ptr(), ids.len(), pos, logits.as_mut_ptr()) })?;
        Ok(logits)
    }

    /// `forward` with every row scored on the device (prompt log-probabilities): row i against `targets[i]` (`FL_SCORE_NO_TARGET`:
    /// none), or -- `targets` `None` -- against `ids[i + 1]`, the last row having none.  The cache ends up as `forward` leaves it; no
    /// token is selected; the distribution is the model's own.
    pub fn forward_score(&self, cache: &mut Cache, ids: &[u32], pos: usize, top_n: usize, targets: Option<&[u32]>) -> Result<ScoredTokens> {
        let t = ids.len();
        if let Some(tg) = targets {
            if tg.len() != t {
                return Err(Error { code: ffi::FL_ERR_BAD_ARGUMENT, message: "forward_score: one target per id".into() });
            }
        }
        let mut lp = vec![0f32; t.max(1)];
        let mut rank = vec![0u32; t.max(1)];
        let mut top_ids = vec![0u32; (t * top_n).max(1)];
        let mut top = vec![0f32; (t * top_n).max(1)];
        let sc = ffi::fl_score {
            struct_size: std::mem::size_of::<ffi::fl_score>() as u32,
            top_n: top_n as i32,
            targets: targets.map(|x| x.as_ptr()).unwrap_or(ptr::null()),
            target_logprob: lp.as_mut_ptr(),
            target_rank: rank.as_mut_ptr(),
            top_ids: if top_n > 0 { top_ids.as_mut_ptr() } else { ptr::null_mut() },
            top_logprobs: if top_n > 0 { top.as_mut_ptr() } else { ptr::null_mut() },
            logits_out: ptr::null_mut(),
            _reserved: [0; 2],
        };
        check(unsafe { ffi::fl_forward_score(self.raw, cache.raw, ids.as_ptr(), t, pos, &sc) })?;
        lp.truncate(t);
        rank.truncate(t);
        top_ids.truncate(t * top_n);
        top.truncate(t * top_n);
        Ok(ScoredTokens { target_logprob: lp, target_rank: rank, top_ids, top_logprobs: top, top_n })
    }

    /// The same forward with ArgMax on the device (ties -> last index, Rust `max_by`).
    pub fn forward_argmax(&self, cache: &mut Cache, ids: &[u32], pos: usize) -> Result<u32> {
        let mut tok = 0u32;
        check(unsafe { ffi::fl_forward_argmax(self.raw, cache.raw, ids.as_ptr(), ids.len(), pos, &mut tok) })?;
        Ok(tok)
    }

    /// Seeded temperature sampling on the device (`temperature < 1e-7`: ArgMax, as candle).
    pub fn forward_sample(&self, cache: &mut Cache, ids: &[u32], pos: usize, s: Sampling) -> Result<u32> {
        let mut tok = 0u32;
        let sp = s.to_ffi();
        check(unsafe { ffi::fl_forward_sample(self.raw, cache.raw, ids.as_ptr(), ids.len(), pos, &sp, &mut tok) })?;
        Ok(tok)
    }

    /// `forward_sample` with top-p / top-k.
    pub fn forward_sample_ex(&self, cache: &mut Cache, ids: &[u32], pos: usize, s: Sampler) -> Result<u32> {
        let mut tok = 0u32;
        let sp = s.to_ffi();
        check(unsafe { ffi::fl_forward_sample_ex(self.raw, cache.raw, ids.as_ptr(), ids.len(), pos, &sp, &mut tok) })?;
        Ok(tok)
    }

    /// `fl_batch_prefill`: `prompts[i]` appended to `caches[i]` at RoPE offset `pos[i]`, all in ONE forward -- per member the result of
    /// `forward_sample_ex` (`None`: ArgMax).  Returns every member's token.  At most 64 members and `FL_PREFILL_CHUNK` tokens in all.
    pub fn prefill_packed(&self, caches: &mut [&mut Cache], prompts: &[&[u32]], pos: &[usize], samplers: &[Option<Sampler>]) -> Result<Vec<u32>> {
        let n = caches.len();
        if prompts.len() != n || pos.len() != n || samplers.len() != n {
            return Err(Error { code: ffi::FL_ERR_BAD_ARGUMENT, message: format!("packed prefill of {} caches: every slice must have that length", n) });
        }
        let raws: Vec<*mut ffi::fl_cache> = caches.iter().map(|c| c.raw).collect();
        let mut ids: Vec<u32> = Vec::new();
        let mut offsets = vec![0usize; n + 1];
        for (i, p) in prompts.iter().enumerate() {
            ids.extend_from_slice(p);
            offsets[i + 1] = ids.len();
        }
        let greedy = Sampler { temperature: 0.0, top_p: 0.0, top_k: 0, seed: 0, draws_done: 0 };
        let sp: Vec<ffi::fl_sampler> = samplers.iter().map(|s| s.unwrap_or(greedy).to_ffi()).collect();
        let mut toks = vec![0u32; n];
        check(unsafe {
            ffi::fl_batch_prefill(self.raw, raws.as_ptr(), n, ids.as_ptr(), offsets.as_ptr(), pos.as_ptr(), sp.as_ptr(), toks.as_mut_ptr(), ptr::null_mut())
        })?;
        Ok(toks)
    }

    /// `fl_batch_embed`: `seqs[i]` appended to `caches[i]` at RoPE offset `pos[i]`, all in ONE forward, and the pooled final hidden
    /// states instead of logits: one vector of `dims` values per member (`Pooling::None`: per token), `dims` = `opts.dimensions` or
    /// the hidden size.  `Mask::Full` needs empty caches and leaves the full-mask model's K/V in them: reset them before decoding.
    pub fn embed_packed(&self, caches: &mut [&mut Cache], seqs: &[&[u32]], pos: &[usize], opts: EmbedOptions) -> Result<Vec<Vec<f32>>> {
        let n = caches.len();
        if seqs.len() != n || pos.len() != n {
            return Err(Error { code: ffi::FL_ERR_BAD_ARGUMENT, message: format!("packed embed of {} caches: every slice must have that length", n) });
        }
        let mut info: ffi::fl_model_info = unsafe { std::mem::zeroed() };
        check(unsafe { ffi::fl_model_get_info(self.raw, &mut info) })?;
        let hidden = info.cfg.hidden_size as usize;
        let dims = if opts.dimensions == 0 { hidden } else { opts.dimensions };
        if dims > hidden {
            return Err(Error { code: ffi::FL_ERR_BAD_ARGUMENT, message: format!("dimensions {} exceeds the hidden size {}", dims, hidden) });
        }
        let raws: Vec<*mut ffi::fl_cache> = caches.iter().map(|c| c.raw).collect();
        let mut ids: Vec<u32> = Vec::new();
        let mut offsets = vec![0usize; n + 1];
        for (i, p) in seqs.iter().enumerate() {
            ids.extend_from_slice(p);
            offsets[i + 1] = ids.len();
        }
        let rows = if opts.pooling == Pooling::None { ids.len() } else { n };
        let e = ffi::fl_embed {
            struct_size: std::mem::size_of::<ffi::fl_embed>() as u32,
            pooling: opts.pooling as i32,
            mask: opts.mask as i32,
            normalize: opts.normalize as i32,
            dimensions: opts.dimensions as i64,
            _reserved: [0; 2],
        };
        let mut out = vec![0f32; (rows * dims).max(1)];
        check(unsafe { ffi::fl_batch_embed(self.raw, raws.as_ptr(), n, ids.as_ptr(), offsets.as_ptr(), pos.as_ptr(), &e, out.as_mut_ptr()) })?;
        Ok((0..rows).map(|r| out[r * dims..(r + 1) * dims].to_vec()).collect())
    }

    /// `fl_batch_verify`: the verify steps `[tokens[i], drafts[i]..]` of `caches[i]` at RoPE offset `pos[i]`, all in ONE forward -- per
    /// member the result of `forward_verify` / its sampled form (`None`: ArgMax; a sampler's `draws_done` is the member's own).  Returns
    /// every member's ids: the accepted drafts followed by the model's own next token.  At most 64 members of at most 15 drafts each.
    pub fn verify_packed(
        &self,
        caches: &mut [&mut Cache],
        tokens: &[u32],
        drafts: &[&[u32]],
        pos: &[usize],
        samplers: &[Option<Sampler>],
    ) -> Result<Vec<Vec<u32>>> {
        let n = caches.len();
        if tokens.len() != n || drafts.len() != n || pos.len() != n || samplers.len() != n {
            return Err(Error { code: ffi::FL_ERR_BAD_ARGUMENT, message: format!("packed verify of {} caches: every slice must have that length", n) });
        }
        let raws: Vec<*mut ffi::fl_cache> = caches.iter().map(|c| c.raw).collect();
        let mut ids: Vec<u32> = Vec::new();
        let mut offsets = vec![0usize; n + 1];
        for i in 0..n {
            ids.push(tokens[i]);
            ids.extend_from_slice(drafts[i]);
            offsets[i + 1] = ids.len();
        }
        let greedy = Sampler { temperature: 0.0, top_p: 0.0, top_k: 0, seed: 0, draws_done: 0 };
        let sp: Vec<ffi::fl_sampler> = samplers.iter().map(|s| s.unwrap_or(greedy).to_ffi()).collect();
        let mut toks = vec![0u32; ids.len().max(1)];
        let mut counts = vec![0usize; n.max(1)];
        check(unsafe {
            ffi::fl_batch_verify(
                self.raw,
                raws.as_ptr(),
                n,
                ids.as_ptr(),
                offsets.as_ptr(),
                pos.as_ptr(),
                sp.as_ptr(),
                toks.as_mut_ptr(),
                counts.as_mut_ptr(),
                ptr::null_mut(),
            )
        })?;
        Ok((0..n).map(|i| toks[offsets[i]..offsets[i] + counts[i]].to_vec()).collect())
    }

    /// `decode` with top-p / top-k.
    pub fn decode_ex(&self, cache: &mut Cache, first_token: u32, pos: usize, n_steps: usize, eos: Option<u32>, s: Sampler) -> Result<Vec<u32>> {
        let mut toks = vec![0u32; n_steps];
        let mut n = 0usize;
        let sp = s.to_ffi();
        check(unsafe {
            ffi::fl_decode_sample_ex(self.raw, cache.raw, first_token, pos, n_steps, eos.map(|e| e as i64).unwrap_or(-1), &sp, toks.as_mut_ptr(), &mut n)
        })?;
        toks.truncate(n);
        Ok(toks)
    }

    /// `decode_ex` with log-probabilities: per emitted token its log-probability under the model's own distribution (temperature 1,
    /// nothing masked -- whatever `s` is) and, with `top_n > 0` (at most `FL_LOGPROBS_MAX_TOP`), the `top_n` most likely ids and
    /// theirs, in the order "logit descending, lower index first".  The tokens are those of `decode_ex`.
    pub fn decode_sample_logprobs(&self, cache: &mut Cache, first_token: u32, pos: usize, n_steps: usize, eos: Option<u32>, s: Sampler,
                                  top_n: usize) -> Result<TokenLogprobs> {
        let mut toks = vec![0u32; n_steps.max(1)];
        let mut token = vec![0f32; n_steps.max(1)];
        let mut top_ids = vec![0u32; (n_steps * top_n).max(1)];
        let mut top = vec![0f32; (n_steps * top_n).max(1)];
        let mut n = 0usize;
        let sp = s.to_ffi();
        let lp = ffi::fl_logprobs {
            struct_size: std::mem::size_of::<ffi::fl_logprobs>() as u32,
            top_n: top_n as i32,
            token_logprob: token.as_mut_ptr(),
            top_ids: if top_n > 0 { top_ids.as_mut_ptr() } else { ptr::null_mut() },
            top_logprobs: if top_n > 0 { top.as_mut_ptr() } else { ptr::null_mut() },
            _reserved: [0; 2],
        };
        check(unsafe {
            ffi::fl_decode_sample_lp(self.raw, cache.raw, first_token, pos, n_steps, eos.map(|e| e as i64).unwrap_or(-1), &sp, toks.as_mut_ptr(), &mut n, &lp)
        })?;
        toks.truncate(n);
        token.truncate(n);
        top_ids.truncate(n * top_n);
        top.truncate(n * top_n);
        Ok(TokenLogprobs { tokens: toks, token_logprob: token, top_ids, top_logprobs: top, top_n })
    }

    /// The loop body of `Model<M>::generate` (mod.rs:411-453) kept on the device; returns the tokens sampled after each
    /// step, shorter than `n_steps` when `eos` was sampled (which is not included).
    pub fn decode(&self, cache: &mut Cache, first_token: u32, pos: usize, n_steps: usize, eos: Option<u32>, sampling: Option<Sampling>) -> Result<Vec<u32>> {
        let mut toks = vec![0u32; n_steps.max(1)];
        let mut n = 0usize;
        let eos = eos.map(|e| e as i64).unwrap_or(-1);
        let rc = match sampling {
            None => unsafe { ffi::fl_decode_greedy(self.raw, cache.raw, first_token, pos, n_steps, eos, toks.as_mut_ptr(), &mut n) },
            Some(s) => {
                let sp = s.to_ffi();
                unsafe { ffi::fl_decode_sample(self.raw, cache.raw, first_token, pos, n_steps, eos, &sp, toks.as_mut_ptr(), &mut n) }
            }
        };
        check(rc)?;
        toks.truncate(n);
        Ok(toks)
    }

    /// `fl_forward_verify`: one forward of `[token, draft..]`; returns the accepted drafts followed by the model's own next token
    /// (which is not cached: it is the `token` of the next call at `pos + returned.len()`).
    pub fn forward_verify(&self, cache: &mut Cache, token: u32, draft: &[u32], pos: usize) -> Result<Vec<u32>> {
        let mut toks = vec![0u32; draft.len() + 1];
        let mut n = 0usize;
        check(unsafe { ffi::fl_forward_verify(self.raw, cache.raw, token, draft.as_ptr(), draft.len(), pos, toks.as_mut_ptr(), &mut n, ptr::null_mut()) })?;
        toks.truncate(n);
        Ok(toks)
    }

    /// `fl_decode_lookup`: the greedy loop of `decode` built from verify steps with prompt-lookup drafts out of
    /// `corpus ++ [first_token] ++ output`; also returns the step / drafted / accepted counts.
    pub fn decode_lookup(
        &self,
        cache: &mut Cache,
        corpus: &[u32],
        first_token: u32,
        pos: usize,
        n_steps: usize,
        eos: Option<u32>,
        opts: Lookup,
    ) -> Result<(Vec<u32>, ffi::fl_spec_stats)> {
        let mut toks = vec![0u32; n_steps.max(1)];
        let mut n = 0usize;
        let mut stats = ffi::fl_spec_stats::default();
        let o = opts.to_ffi();
        check(unsafe {
            ffi::fl_decode_lookup(
                self.raw,
                cache.raw,
                corpus.as_ptr(),
                corpus.len(),
                first_token,
                pos,
                n_steps,
                eos.map(|e| e as i64).unwrap_or(-1),
                &o,
                toks.as_mut_ptr(),
                &mut n,
                &mut stats,
            )
        })?;
        toks.truncate(n);
        Ok((toks, stats))
    }

    /// `fl_decode_lookup_ex`: the sampled loop of `decode_ex` built from verify steps -- row `i` of a step is drawn with word
    /// `s.draws_done + emitted + i` of the seeded stream and accepted while the draws equal the drafts, so token `k` is drawn with
    /// word `k` as in the plain loop.  `s.temperature < 1e-7` is `decode_lookup`.
    pub fn decode_lookup_sampled(
        &self,
        cache: &mut Cache,
        corpus: &[u32],
        first_token: u32,
        pos: usize,
        n_steps: usize,
        eos: Option<u32>,
        opts: Lookup,
        s: Sampler,
    ) -> Result<(Vec<u32>, ffi::fl_spec_stats)> {
        let mut toks = vec![0u32; n_steps.max(1)];
        let mut n = 0usize;
        let mut stats = ffi::fl_spec_stats::default();
        let o = opts.to_ffi();
        let sp = s.to_ffi();
        check(unsafe {
            ffi::fl_decode_lookup_ex(
                self.raw,
                cache.raw,
                corpus.as_ptr(),
                corpus.len(),
                first_token,
                pos,
                n_steps,
                eos.map(|e| e as i64).unwrap_or(-1),
                &o,
                &sp,
                toks.as_mut_ptr(),
                &mut n,
                &mut stats,
            )
        })?;
        toks.truncate(n);
        Ok((toks, stats))
    }

    /// `fl_decode_lookup_lp`: `decode_lookup_sampled` for a FULL request -- the cache may have logit rules (`frequency_penalty`,
    /// `presence_penalty`, `logit_bias`) and / or a guide (`response_format`, strict tool calls) installed, and `top_n` (`None`: no
    /// log-probs) asks for each emitted token's log-probability under the model's own distribution.  Row `i` of a verify step sees
    /// the rules table and the guide state the plain loop (`decode_sample_logprobs` on the same cache) would hold at that step, so
    /// the tokens, the table and the guide state afterwards are the plain loop's.  `s.temperature < 1e-7`: ArgMax.
    pub fn decode_lookup_request(
        &self,
        cache: &mut Cache,
        corpus: &[u32],
        first_token: u32,
        pos: usize,
        n_steps: usize,
        eos: Option<u32>,
        opts: Lookup,
        s: Sampler,
        top_n: Option<usize>,
    ) -> Result<(TokenLogprobs, ffi::fl_spec_stats)> {
        let k = top_n.unwrap_or(0);
        let mut toks = vec![0u32; n_steps.max(1)];
        let mut token = vec![0f32; n_steps.max(1)];
        let mut top_ids = vec![0u32; (n_steps * k).max(1)];
        let mut top = vec![0f32; (n_steps * k).max(1)];
        let mut n = 0usize;
        let mut stats = ffi::fl_spec_stats::default();
        let o = opts.to_ffi();
        let sp = s.to_ffi();
        let lp = ffi::fl_logprobs {
            struct_size: std::mem::size_of::<ffi::fl_logprobs>() as u32,
            top_n: k as i32,
            token_logprob: token.as_mut_ptr(),
            top_ids: if k > 0 { top_ids.as_mut_ptr() } else { ptr::null_mut() },
            top_logprobs: if k > 0 { top.as_mut_ptr() } else { ptr::null_mut() },
            _reserved: [0; 2],
        };
        check(unsafe {
            ffi::fl_decode_lookup_lp(
                self.raw,
                cache.raw,
                corpus.as_ptr(),
                corpus.len(),
                first_token,
                pos,
                n_steps,
                eos.map(|e| e as i64).unwrap_or(-1),
                &o,
                &sp,
                if top_n.is_some() { &lp } else { ptr::null() },
                toks.as_mut_ptr(),
                &mut n,
                &mut stats,
            )
        })?;
        toks.truncate(n);
        token.truncate(if top_n.is_some() { n } else { 0 });
        top_ids.truncate(n * k);
        top.truncate(n * k);
        Ok((TokenLogprobs { tokens: toks, token_logprob: token, top_ids, top_logprobs: top, top_n: k }, stats))
    }

    pub fn synchronize(&self) -> Result<()> {
        check(unsafe { ffi::fl_synchronize(self.raw) })
    }
}

/// `fl_cache*`: the KV cache of one request / stream.  Not `Sync`: one forward at a time per cache.
pub struct Cache {
    raw: *mut ffi::fl_cache,
}
unsafe impl Send for Cache {}
impl Drop for Cache {
    fn drop(&mut self) {
        unsafe { ffi::fl_cache_destroy(self.raw) };
    }
}
impl Cache {
    /// `clear_kv_cache` (mistral.rs:220, qwen.rs:148).
    pub fn reset(&mut self) {
        unsafe { ffi::fl_cache_reset(self.raw) };
    }
    /// `fl_cache_truncate`: forget everything from position `len` on (an error beyond the cached length).
    pub fn truncate(&mut self, len: usize) -> Result<()> {
        check(unsafe { ffi::fl_cache_truncate(self.raw, len) })
    }
    /// `fl_cache_copy_prefix`: this cache forgets what it holds and takes the first `n` cached positions of `src` (a cache of the
    /// same model; `src` is unchanged).  Afterwards `len() == n` and the next call appends at `n`, as if this cache had computed
    /// those positions itself.  Errors: `n` beyond `src.len()` or caches of two models (`FL_ERR_BAD_ARGUMENT`), `n` beyond
    /// `capacity()` (`FL_ERR_SEQ_OVERFLOW`).
    pub fn copy_prefix_from(&mut self, src: &Cache, n: usize) -> Result<()> {
        check(unsafe { ffi::fl_cache_copy_prefix(self.raw, src.raw as *const ffi::fl_cache, n) })
    }
    /// `fl_cache_set_logit_rules`: from now on every call that selects a token for this cache applies `rules` on the device -- inside
    /// the replayed decode step -- to the row it selects from.  `prompt_ids` mark ids as "seen in the prompt" (repetition penalty),
    /// `output_ids` seed the output counts, which `decode*` and the batch decode loops then keep themselves.  Log-probs and
    /// `forward` logits stay the model's own.  Errors: an id beyond the vocabulary, a duplicate bias id, a NaN or out-of-range
    /// scalar (`FL_ERR_BAD_ARGUMENT`); a tensor-parallel model (`FL_ERR_UNSUPPORTED`).
    pub fn set_logit_rules(&mut self, model: &Model, rules: &LogitRules, prompt_ids: &[u32], output_ids: &[u32]) -> Result<()> {
        let (ids, values): (Vec<u32>, Vec<f32>) = rules.logit_bias.iter().copied().unzip();
        let r = ffi::fl_logit_rules {
            struct_size: std::mem::size_of::<ffi::fl_logit_rules>() as u32,
            n_bias: ids.len() as u32,
            bias_ids: if ids.is_empty() { ptr::null() } else { ids.as_ptr() },
            bias_values: if values.is_empty() { ptr::null() } else { values.as_ptr() },
            repetition_penalty: rules.repetition_penalty,
            frequency_penalty: rules.frequency_penalty,
            presence_penalty: rules.presence_penalty,
            _reserved: [0; 2],
        };
        let p = if prompt_ids.is_empty() { ptr::null() } else { prompt_ids.as_ptr() };
        let o = if output_ids.is_empty() { ptr::null() } else { output_ids.as_ptr() };
        check(unsafe { ffi::fl_cache_set_logit_rules(model.raw, self.raw, &r, p, prompt_ids.len(), o, output_ids.len()) })
    }
    /// Removes the rules: the cache runs exactly what it ran before they were installed.
    pub fn clear_logit_rules(&mut self, model: &Model) -> Result<()> {
        check(unsafe { ffi::fl_cache_set_logit_rules(model.raw, self.raw, ptr::null(), ptr::null(), 0, ptr::null(), 0) })
    }
    /// `fl_cache_set_guide`: from now on every call that selects a token for this cache selects among the ids the automaton allows in
    /// its current state -- masked on the device, inside the replayed decode step -- and moves along the selected token's edge.
    /// `state` is the state in which the next selected token is looked up.  `truncate`, `reset` and `copy_prefix_from` leave guide and
    /// state alone: after a rollback set the state again.  `FL_ERR_UNSUPPORTED`: a tensor-parallel model.
    pub fn set_guide(&mut self, model: &Model, guide: &Guide, state: u32) -> Result<()> {
        check(unsafe { ffi::fl_cache_set_guide(model.raw, self.raw, guide.raw, state) })
    }
    /// Removes the guide: the cache runs exactly what it ran before one was installed.
    pub fn clear_guide(&mut self, model: &Model) -> Result<()> {
        check(unsafe { ffi::fl_cache_set_guide(model.raw, self.raw, ptr::null_mut(), 0) })
    }
    /// `fl_cache_guide_state`.
    pub fn guide_state(&self) -> Result<u32> {
        let mut s = 0u32;
        check(unsafe { ffi::fl_cache_guide_state(self.raw as *const ffi::fl_cache, &mut s) })?;
        Ok(s)
    }
    pub fn len(&self) -> usize {
        unsafe { ffi::fl_cache_len(self.raw) }
    }
    pub fn is_empty(&self) -> bool {
        self.len() == 0
    }
    pub fn capacity(&self) -> usize {
        unsafe { ffi::fl_cache_capacity(self.raw) }
    }
}

/// `fl_batch*`: up to 64 caches of one model decoded together (one read of the weights per step for all of them).
pub struct Batch<'a> {
    raw: *mut ffi::fl_batch,
    n: usize,
    _caches: std::marker::PhantomData<&'a mut Cache>,
}
impl<'a> Drop for Batch<'a> {
    fn drop(&mut self) {
        unsafe { ffi::fl_batch_destroy(self.raw) };
    }
}
impl<'a> Batch<'a> {
    pub fn new(model: &Model, caches: &'a mut [Cache]) -> Result<Batch<'a>> {
        let raws: Vec<*mut ffi::fl_cache> = caches.iter().map(|c| c.raw).collect();
        let mut raw: *mut ffi::fl_batch = ptr::null_mut();
        check(unsafe { ffi::fl_batch_create(model.raw, raws.as_ptr(), raws.len(), &mut raw) })?;
        Ok(Batch { raw, n: raws.len(), _caches: std::marker::PhantomData })
    }

    /// `n_steps` greedy / sampled steps for every sequence; row `i` holds sequence `i`'s tokens (cut at its EOS).
    pub fn decode(&mut self, first_tokens: &[u32], pos: &[usize], n_steps: usize, eos: Option<u32>, sampling: Option<Sampling>) -> Result<Vec<Vec<u32>>> {
        if first_tokens.len() != self.n || pos.len() != self.n {
            return Err(Error { code: ffi::FL_ERR_BAD_ARGUMENT, message: format!("batch of {} sequences, got {} tokens / {} positions", self.n, first_tokens.len(), pos.len()) });
        }
        let mut toks = vec![0u32; self.n * n_steps.max(1)];
        let mut n_out = vec![0usize; self.n];
        let sp = sampling.map(|s| s.to_ffi());
        let spp = sp.as_ref().map(|s| s as *const ffi::fl_sampling).unwrap_or(ptr::null());
        check(unsafe {
            ffi::fl_batch_decode(self.raw, first_tokens.as_ptr(), pos.as_ptr(), n_steps, eos.map(|e| e as i64).unwrap_or(-1), spp, toks.as_mut_ptr(), n_out.as_mut_ptr())
        })?;
        Ok((0..self.n).map(|i| toks[i * n_steps..i * n_steps + n_out[i]].to_vec()).collect())
    }

    /// ... with every sequence's own EOS and sampler (`None`: ArgMax): one batch mixes ArgMax, `Sampling::All` and top-p / top-k.
    pub fn decode_each(&mut self, first_tokens: &[u32], pos: &[usize], n_steps: usize, eos: &[Option<u32>], samplers: &[Option<Sampler>]) -> Result<Vec<Vec<u32>>> {
        if first_tokens.len() != self.n || pos.len() != self.n || eos.len() != self.n || samplers.len() != self.n {
            return Err(Error { code: ffi::FL_ERR_BAD_ARGUMENT, message: format!("batch of {} sequences: every slice must have that length", self.n) });
        }
        let mut toks = vec![0u32; self.n * n_steps.max(1)];
        let mut n_out = vec![0usize; self.n];
        let greedy = Sampler { temperature: 0.0, top_p: 0.0, top_k: 0, seed: 0, draws_done: 0 };
        let sp: Vec<ffi::fl_sampler> = samplers.iter().map(|s| s.unwrap_or(greedy).to_ffi()).collect();
        let e: Vec<i64> = eos.iter().map(|x| x.map(|v| v as i64).unwrap_or(-1)).collect();
        check(unsafe {
            ffi::fl_batch_decode_each_ex(self.raw, first_tokens.as_ptr(), pos.as_ptr(), n_steps, e.as_ptr(), sp.as_ptr(), toks.as_mut_ptr(), n_out.as_mut_ptr())
        })?;
        Ok((0..self.n).map(|i| toks[i * n_steps..i * n_steps + n_out[i]].to_vec()).collect())
    }
}

/// The encoder's GELU form (`fl_activation`).  `Tanh` is candle's `Tensor::gelu`, what the reference runs (embeddings.rs:229-231);
/// `Erf` is the exact form HF BERT checkpoints were trained with.
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
#[repr(i32)]
pub enum Activation {
    GeluTanh = ffi::FL_ACT_GELU_TANH,
    GeluErf = ffi::FL_ACT_GELU_ERF,
}

/// The fields of the reference's `BertConfig` (src/models/embeddings.rs:46-54) plus what the reference takes from elsewhere or
/// hard-wires: `vocab_size` (the tokenizer's, :301-303), the GELU form, HF's token-type row 0 (the reference never adds it,
/// :370-378) and the workspace size (`max_batch_tokens` 0: the library's default, 4096).
#[derive(Clone, Debug)]
pub struct EncoderConfig {
    pub hidden_size: usize,
    pub num_attention_heads: usize,
    pub num_hidden_layers: usize,
    pub intermediate_size: usize,
    pub max_position_embeddings: usize,
    pub layer_norm_eps: f64,
    pub vocab_size: usize,
    pub activation: Activation,
    pub add_token_type0: bool,
    pub max_batch_tokens: usize,
}

impl EncoderConfig {
    pub fn to_ffi(&self) -> ffi::fl_encoder_config {
        ffi::fl_encoder_config {
            struct_size: std::mem::size_of::<ffi::fl_encoder_config>() as u32,
            activation: self.activation as i32,
            add_token_type0: self.add_token_type0 as i32,
            _pad: 0,
            hidden_size: self.hidden_size as i64,
            intermediate_size: self.intermediate_size as i64,
            num_hidden_layers: self.num_hidden_layers as i64,
            num_attention_heads: self.num_attention_heads as i64,
            max_position_embeddings: self.max_position_embeddings as i64,
            vocab_size: self.vocab_size as i64,
            max_batch_tokens: self.max_batch_tokens as i64,
            layer_norm_eps: self.layer_norm_eps,
            _reserved: [0; 2],
        }
    }
}

/// `fl_encoder*`: the BERT / MiniLM encoder forward on one GPU (the reference's `MiniLMModel`, which runs on the CPU).  The library
/// serialises submission per encoder, so a shared reference may be used from several threads.
pub struct Encoder {
    raw: *mut ffi::fl_encoder,
    hidden: usize,
}
// SAFETY: submission is serialised per encoder and every entry sets its HIP device itself (include/fastllm_mi355x.h).
unsafe impl Send for Encoder {}
unsafe impl Sync for Encoder {}

impl Drop for Encoder {
    fn drop(&mut self) {
        unsafe { ffi::fl_encoder_release(self.raw) };
    }
}

impl Encoder {
    /// Tensor names as in the checkpoint, without a `bert.` prefix (embeddings.rs:298-327).
    pub fn new(cfg: &EncoderConfig, tensors: &[TensorView<'_>], compute: DType, device_id: i32) -> Result<Encoder> {
        let names: Vec<CString> = tensors
            .iter()
            .map(|t| CString::new(t.name).map_err(|_| Error { code: ffi::FL_ERR_BAD_ARGUMENT, message: format!("tensor name {:?} contains NUL", t.name) }))
            .collect::<Result<_>>()?;
        let mut descr = Vec::with_capacity(tensors.len());
        for (t, name) in tensors.iter().zip(&names) {
            if t.shape.len() > 4 {
                return Err(Error { code: ffi::FL_ERR_SHAPE_MISMATCH, message: format!("tensor {} has rank {}", t.name, t.shape.len()) });
            }
            let mut shape = [0i64; 4];
            for (d, s) in shape.iter_mut().zip(t.shape) {
                *d = *s as i64;
            }
            descr.push(ffi::fl_tensor { name: name.as_ptr(), dtype: t.dtype as i32, ndim: t.shape.len() as i32, shape, data: t.data, device: t.device, _pad: 0 });
        }
        let c = cfg.to_ffi();
        let mut raw: *mut ffi::fl_encoder = ptr::null_mut();
        // SAFETY: every pointer is valid for the duration of the call; the library copies what it keeps.
        check(unsafe { ffi::fl_encoder_create(&c, descr.as_ptr(), descr.len(), compute as i32, device_id, &mut raw) })?;
        Ok(Encoder { raw, hidden: cfg.hidden_size })
    }

    /// The model's `hidden_size` (the reference's `embedding_size()` hard-codes 384, embeddings.rs:453-455).
    pub fn embedding_size(&self) -> usize {
        self.hidden
    }

    /// `MiniLMModel::forward` (embeddings.rs:380-393): last hidden states of one sequence, row-major `[ids.len()][hidden_size]`.
    pub fn hidden(&self, ids: &[u32]) -> Result<Vec<f32>> {
        let mut out = vec![0f32; ids.len() * self.hidden];
        check(unsafe { ffi::fl_encoder_hidden(self.raw, ids.as_ptr(), ids.len(), out.as_mut_ptr()) })?;
        Ok(out)
    }

    /// `EmbeddingModel::embed` (embeddings.rs:396-447) behind the tokenizer, for many sequences in one packed call: the
    /// L2-normalised mean of each sequence's last hidden states.
    pub fn embed(&self, seqs: &[&[u32]]) -> Result<Vec<Vec<f32>>> {
        let mut ids = Vec::new();
        let mut offsets = vec![0usize];
        for s in seqs {
            ids.extend_from_slice(s);
            offsets.push(ids.len());
        }
        let mut flat = vec![0f32; seqs.len() * self.hidden];
        check(unsafe { ffi::fl_encoder_embed(self.raw, ids.as_ptr(), offsets.as_ptr(), seqs.len(), flat.as_mut_ptr()) })?;
        Ok(flat.chunks(self.hidden.max(1)).map(|c| c.to_vec()).collect())
    }
}

/// The encoder's unmasked ragged attention kernel alone (`fl_op_encoder_attention`) on f32 inputs: `q` / `k` / `v` are
/// `[sum(lengths)][heads * head_dim]`.
pub fn op_encoder_attention_f32(q: &[f32], k: &[f32], v: &[f32], lengths: &[usize], heads: usize, head_dim: usize) -> Result<Vec<f32>> {
    let total: usize = lengths.iter().sum();
    if q.len() != total * heads * head_dim || k.len() != q.len() || v.len() != q.len() {
        return Err(Error { code: ffi::FL_ERR_BAD_ARGUMENT, message: format!("q / k / v must hold {} rows of {} values", total, heads * head_dim) });
    }
    let mut offsets = vec![0usize];
    for l in lengths {
        offsets.push(offsets[offsets.len() - 1] + l);
    }
    let mut out = vec![0f32; q.len()];
    check(unsafe {
        ffi::fl_op_encoder_attention(
            q.as_ptr() as *const c_void,
            k.as_ptr() as *const c_void,
            v.as_ptr() as *const c_void,
            offsets.as_ptr(),
            lengths.len(),
            heads as i64,
            head_dim as i64,
            ffi::FL_DTYPE_F32,
            out.as_mut_ptr(),
        )
    })?;
    Ok(out)
}

/// Number of HIP devices the library sees (0 without a GPU: `Model::new` then fails with `FL_ERR_NO_DEVICE`; there is
/// no CPU path).
pub fn device_count() -> usize {
    let mut n = 0;
    let _ = unsafe { ffi::fl_device_count(&mut n) };
    n.max(0) as usize
}

pub fn abi_version() -> i32 {
    unsafe { ffi::fl_abi_version() }
}
