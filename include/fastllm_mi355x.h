/*
 * fastllm_mi355x.h -- C ABI of the MI355X (gfx950 / CDNA4) decoder forward-pass backend
 * for FastLLM (lukehinds/fastllm).
 *
 * This is the drop-in boundary for ONE hot path of the reference: the batch-1, KV-cached
 * causal-LM forward pass behind
 *     trait ModelInitializer { initialize_model; initialize_cache; forward }
 *     (/root/reference/src/models/model_initializer.rs:6-22)
 * for the three families the reference registers (LlamaWithConfig llama.rs:94-150,
 * MistralWithConfig mistral.rs:156-237, QwenWithConfig qwen.rs:89-152).  The reference has no
 * FFI today (no extern "C" anywhere); its arithmetic is delegated to candle.  A Rust
 * `impl ModelInitializer for Mi355xWithConfig` binds exactly the entry points below
 * (binding shown in INTEGRATION.md).
 *
 * Conventions
 *   - every entry returns an fl_status (0 = OK, negative = error); fl_last_error() gives a
 *     thread-local message (anyhow::Error analogue).  Nothing aborts or throws across the ABI: every
 *     entry is an exception barrier (std::bad_alloc -> FL_ERR_OOM, anything else -> FL_ERR_HIP).
 *   - plain pointers and sizes only; opaque handles for model and cache.
 *   - thread-safe: any number of threads may call fl_forward on ONE model with DISTINCT caches
 *     (the reference's streaming path does that, mod.rs:137-238); submission is serialised
 *     per model.  Every entry sets the HIP device itself.
 *   - the library never falls back to a CPU path: without a usable gfx950 device
 *     fl_model_create fails with FL_ERR_NO_DEVICE.
 */
#ifndef FASTLLM_MI355X_H
#define FASTLLM_MI355X_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FL_ABI_VERSION 2

typedef enum fl_status {
    FL_OK = 0,
    FL_ERR_BAD_CONFIG = -1,      /* reference: assert!/expect panics, mistral.rs:109-127, qwen.rs:32-37 */
    FL_ERR_MISSING_TENSOR = -2,  /* candle VarBuilder "cannot find tensor" */
    FL_ERR_SHAPE_MISMATCH = -3,
    FL_ERR_OOM = -4,
    FL_ERR_HIP = -5,
    FL_ERR_RCCL = -6,
    FL_ERR_SEQ_OVERFLOW = -7,
    FL_ERR_BAD_ARGUMENT = -8,
    FL_ERR_NO_DEVICE = -9,
    FL_ERR_UNSUPPORTED = -10
} fl_status;

/* ModelArchitecture::get_family (llama.rs:153, mistral.rs:240, qwen.rs:174) */
typedef enum fl_family { FL_FAMILY_LLAMA = 0, FL_FAMILY_MISTRAL = 1, FL_FAMILY_QWEN2 = 2 } fl_family;

/* candle_core::DType subset the reference can hand over (dtype_utils.rs:10-23) */
typedef enum fl_dtype { FL_DTYPE_F32 = 0, FL_DTYPE_BF16 = 1, FL_DTYPE_F16 = 2 } fl_dtype;

/* The fields of the reference's ConfigFile / BaseModelConfig (llama.rs:18-29,
 * mistral.rs:80-92, config.rs:6-18).  A 0 in an optional field means "absent from
 * config.json" and takes the reference's default:
 *   num_key_value_heads  -> num_attention_heads        (llama.rs:39, mistral.rs:97, qwen.rs:45)
 *   rope_theta           -> 10000                      (llama.rs:41, mistral.rs:137, qwen.rs:47)
 *   max_position_embeddings -> 4096 llama / 32768 mistral, qwen (llama.rs:47, mistral.rs:138, qwen.rs:48)
 *   sliding_window       -> 4096 mistral, qwen; unused for llama (mistral.rs:139, qwen.rs:49)
 * head_dim is hidden_size / num_attention_heads (mistral.rs:67-76, config.rs:32-44); it is not
 * a config field in the reference and is validated, not passed.  Every even head_dim up to 128 is supported, as the
 * reference accepts them (config.rs:31-43): the kernels are built for 64 and 128 (TinyLlama; Mistral-7B, Qwen2-7B and every
 * Llama-2/3 size) and any other value -- 48, 80, 96, 100 (OpenLLaMA-3B) ... -- runs as the next of the two, with zero
 * weight rows between the halves of every head (fl_model_info.head_dim still reports the model's).  REFUSED with
 * FL_ERR_UNSUPPORTED at fl_model_create: head_dim above 128, and hidden_size that is not a multiple of 8; an odd
 * head_dim is FL_ERR_BAD_CONFIG, as in the reference. */
typedef struct fl_config {
    int32_t family;                 /* fl_family */
    int32_t qkv_bias;               /* 1 for Qwen2 (q/k/v_proj.bias tensors), else 0 */
    int64_t hidden_size;
    int64_t intermediate_size;
    int64_t vocab_size;
    int64_t num_hidden_layers;
    int64_t num_attention_heads;
    int64_t num_key_value_heads;
    int64_t max_position_embeddings;
    int64_t sliding_window;
    double  rms_norm_eps;
    double  rope_theta;
} fl_config;

/* One entry of initialize_model's HashMap<String, Tensor> (model_initializer.rs:12).
 * Borrowed for the duration of fl_model_create only; the library copies, shards and
 * re-lays-out into HBM.  `device` < 0: `data` is host memory; >= 0: `data` is a device
 * pointer on that HIP device (the reference loads safetensors straight onto `device`,
 * huggingface.rs:88,125); fl_model_create synchronises the devices before it reads such
 * tensors, so work still in flight on the caller's streams is waited for. */
typedef struct fl_tensor {
    const char *name;               /* HF name, e.g. "model.layers.0.self_attn.q_proj.weight" */
    int32_t dtype;                  /* fl_dtype */
    int32_t ndim;
    int64_t shape[4];
    const void *data;
    int32_t device;
    int32_t _pad;
} fl_tensor;

/* Tensor-parallel placement.  New capability (the reference is single-device, README.md:149). */
typedef enum fl_tp_mode {
    FL_TP_NONE = 0,                 /* one GPU: device_ids[0] (or device 0 if NULL) */
    FL_TP_SINGLE_PROCESS = 1,       /* this process drives tp_size GPUs (device_ids[tp_size]); the
                                       shape of the reference's one-process server (main.rs:128).  Decode
                                       collectives are one-shot pushes over peer pointers, one hipGraph per
                                       shard; RCCL group calls carry the large prefill collectives */
    FL_TP_MULTI_PROCESS = 2,        /* one process per GPU: this process is tp_rank of tp_size.  With a
                                       unique_id it joins that RCCL communicator (large prefill
                                       collectives) and connects the peer inboxes for the small decode
                                       collectives by itself; with unique_id == NULL there is no RCCL and
                                       the host connects the inboxes: fl_comm_ipc_export / _connect */
    FL_TP_EMULATED = 3              /* tp_size shards on ONE GPU, collectives done locally: lets a
                                       single-GPU box verify the sharded kernels (tests only) */
} fl_tp_mode;

#define FL_UNIQUE_ID_BYTES 128
typedef struct fl_parallel {
    int32_t mode;                   /* fl_tp_mode */
    int32_t tp_size;
    int32_t tp_rank;                /* FL_TP_MULTI_PROCESS only */
    int32_t n_device_ids;
    const int32_t *device_ids;
    const void *unique_id;          /* FL_TP_MULTI_PROCESS: FL_UNIQUE_ID_BYTES from fl_comm_unique_id */
} fl_parallel;

typedef struct fl_model fl_model;
typedef struct fl_cache fl_cache;

int         fl_abi_version(void);
const char *fl_last_error(void);
int         fl_device_count(int *count);
/* ncclGetUniqueId; rank 0 calls it and ships the bytes to the other ranks out of band */
int         fl_comm_unique_id(void *out /* FL_UNIQUE_ID_BYTES */);

/* ModelInitializer::initialize_model(&Config, HashMap<String,Tensor>, DType, &Device)
 * (model_initializer.rs:10-17; call site huggingface.rs:135).  compute_dtype: FL_DTYPE_BF16 is
 * the reference's hard-wired dtype (main.rs:120); FL_DTYPE_F32 is the fp32 parity mode. */
int fl_model_create(const fl_config *cfg, const fl_tensor *tensors, size_t n_tensors,
                    int32_t compute_dtype, const fl_parallel *par, fl_model **out);

/* Weight format of the decode step (fl_model_create_opts).  FL_WEIGHTS_E4M3_ROW: the single-stream decode step (T = 1) reads its
 * projection weights (q/k/v, o, gate/up, down, lm_head) as FP8: W'[n,k] = s[n] * q[n,k], q OCP e4m3fn, s[n] = 2^e one fp32 scale
 * per output row, e the smallest integer with absmax(W[n,:]) / 2^e <= 448 (all-zero row: s = 1), q = RNE_e4m3(W / s).  s * q is
 * exact in bf16, so the model IS the bf16 model whose weights are W': prompts (T > 1) and fl_batch_* steps run the bf16 kernels on
 * a bf16 image of W', and every path sees the same weights.  Both images are kept: weight memory is 1.5x a bf16 model's -- this
 * mode buys decode speed (half the bytes of the weight stream), not capacity.  Embedding and norm weights stay as they are.
 * REFUSED: compute_dtype other than BF16, tp_size > 1 (any mode), a model whose fused decode step is off (FL_FUSED=0, hidden_size
 * above 6144), hidden_size not a multiple of 16 -> FL_ERR_UNSUPPORTED; an unknown decode_weights or a struct_size that is not
 * sizeof(fl_model_options) -> FL_ERR_BAD_ARGUMENT.  All but the fused-step one are decided before the device probe. */
typedef enum fl_weight_format { FL_WEIGHTS_COMPUTE_DTYPE = 0, FL_WEIGHTS_E4M3_ROW = 1 } fl_weight_format;
typedef struct fl_model_options {
    uint32_t struct_size;           /* sizeof(fl_model_options) */
    int32_t  decode_weights;        /* fl_weight_format */
    int64_t  _reserved[3];          /* 0 */
} fl_model_options;
/* fl_model_create with options; opts == NULL is fl_model_create. */
int fl_model_create_opts(const fl_config *cfg, const fl_tensor *tensors, size_t n_tensors, int32_t compute_dtype,
                         const fl_parallel *par, const fl_model_options *opts, fl_model **out);

/* FL_TP_MULTI_PROCESS: the decode step's two [h] fp32 all-reduces per layer and the logits all-gather
 * are one-shot pushes into inboxes that every rank maps from every peer's HBM over xGMI (new
 * capability; the reference is single-device, README.md:149).  A model created with a unique_id
 * wires them itself over RCCL.  Otherwise: every rank exports its inbox handle, the host all-gathers
 * the tp handles out of band (rank order) and every rank connects before its first forward.
 * Connected groups with one GPU per rank exchange the all-reduces inside the o_proj / down_proj GEMV epilogues
 * (fl_model_info.fused_all_reduce); waits for a peer are bounded (FL_AR_TIMEOUT_MS) and end in FL_ERR_RCCL. */
#define FL_IPC_HANDLE_BYTES 64
int fl_comm_ipc_export(fl_model *m, void *handle_out /* FL_IPC_HANDLE_BYTES */);
int fl_comm_ipc_connect(fl_model *m, const void *handles /* tp_size * FL_IPC_HANDLE_BYTES */);
/* Clone for the streaming path (mod.rs:155,181,207) is a refcount bump. */
void fl_model_retain(fl_model *m);
void fl_model_release(fl_model *m);

typedef struct fl_model_info {
    fl_config cfg;                  /* defaults resolved */
    int64_t head_dim;
    int32_t compute_dtype;
    int32_t tp_size;
    int64_t weight_bytes_per_token; /* algorithmic HBM bytes a decode step reads from weights (whole model); FL_WEIGHTS_E4M3_ROW: what
                                       that step really streams -- 1 byte per projection weight + 4 per projection row */
    int64_t kv_bytes_per_position;  /* K+V bytes one cached position adds to a decode step */
    int64_t hbm_bytes_allocated;    /* this process, all shards (FL_WEIGHTS_E4M3_ROW: the e4m3 bytes, the scales AND the bf16 image) */
    int32_t small_collectives;      /* decode collectives: 0 none (tp 1), 1 RCCL, 2 one-shot peer inboxes, 3 local (emulated) */
    int32_t fused_all_reduce;       /* 1: decode all-reduces ride in the o_proj / down_proj GEMV epilogues (no kernel of their own) */
    int32_t rccl_ranks;             /* ncclCommCount of this rank's RCCL communicator; 0: no communicator (tp 1, emulated, IPC-only groups) */
    int32_t decode_weights;         /* fl_weight_format the decode step streams */
} fl_model_info;
int fl_model_get_info(const fl_model *m, fl_model_info *out);

/* ModelInitializer::initialize_cache(&Device, DType) (model_initializer.rs:19; per request,
 * mod.rs:370).  The reference's version cannot see the model (hard-coded TinyLlama dims,
 * llama.rs:125-145); here the cache is derived from the model and owned by the caller. */
int    fl_cache_create(fl_model *m, size_t max_seq, fl_cache **out);
void   fl_cache_reset(fl_cache *c);          /* clear_kv_cache (mistral.rs:220, qwen.rs:148) */
size_t fl_cache_len(const fl_cache *c);
size_t fl_cache_capacity(const fl_cache *c);
void   fl_cache_destroy(fl_cache *c);

/* ModelInitializer::forward(&self, input[1,T] u32, pos, &mut cache) -> logits
 * (model_initializer.rs:21; call sites mod.rs:402-405,446-451).
 *   ids[T]      token ids (batch is always 1, mod.rs:283-291)
 *   pos         RoPE offset of ids[0].  Keys/values are APPENDED at fl_cache_len (candle's
 *               Tensor::cat), so a caller that passes the reference's call counter for
 *               Mistral/Qwen (mistral.rs:226,234) gets the reference's results.
 *   logits_out  host, [vocab_size] fp32: the LAST position's logits, i.e. what the caller takes
 *               with logits.get(0)?.flatten_all()? (mod.rs:305,421) after to_dtype(F32).
 * Blocking: returns when logits are on the host. */
int fl_forward(fl_model *m, fl_cache *c, const uint32_t *ids, size_t T, size_t pos, float *logits_out);

/* Same forward, but LogitsProcessor ArgMax (temperature < 1e-7; ties -> LAST maximal index,
 * Rust Iterator::max_by) is evaluated on the device and only the token id comes back. */
int fl_forward_argmax(fl_model *m, fl_cache *c, const uint32_t *ids, size_t T, size_t pos, uint32_t *token_out);

/* The body of the greedy loop of Model<M>::generate (mod.rs:411-453) kept on the device:
 * starting from `first_token` (already sampled by the caller from the prefill logits), run
 * n_steps x { forward([tok], pos) ; tok = argmax ; pos += pos_stride } with no host round trip.
 * tokens_out[i] is the token sampled after step i.  Stops early (n_out < n_steps) when the
 * sampled token == eos (eos < 0: never).  pos_stride is 1; pos is whatever offset the caller's
 * position mode dictates. */
int fl_decode_greedy(fl_model *m, fl_cache *c, uint32_t first_token, size_t pos, size_t n_steps,
                     int64_t eos, uint32_t *tokens_out, size_t *n_out);

/* LogitsProcessor::new(seed, Some(temperature), None) + .sample() (mod.rs:373-374,425-428) on the device.
 * temperature < 1e-7 is ArgMax, as in candle.  Otherwise Sampling::All: softmax(logits / temperature) in
 * fp32, then rand 0.8's WeightedIndex<f32> driven by StdRng::seed_from_u64(seed) (ChaCha12); one u32 word of
 * the stream is consumed per sampled token.  The reference builds a fresh processor with seed 0 per
 * request, samples the first token from the prefill logits and goes on in the loop: here that is
 *   fl_forward_sample(.., {t, 0, 0}, &tok);  fl_decode_sample(.., tok, pos, n, eos, {t, 0, 1}, ..)
 * (draws_done = words already consumed, so one request may span several calls). */
typedef struct fl_sampling {
    double   temperature;
    uint64_t seed;
    uint64_t draws_done;
} fl_sampling;
int fl_forward_sample(fl_model *m, fl_cache *c, const uint32_t *ids, size_t T, size_t pos,
                      const fl_sampling *sampling, uint32_t *token_out);
int fl_decode_sample(fl_model *m, fl_cache *c, uint32_t first_token, size_t pos, size_t n_steps, int64_t eos,
                     const fl_sampling *sampling, uint32_t *tokens_out, size_t *n_out);

/* The same two calls with candle's other sampling modes (generation::Sampling::TopP / TopK / TopKThenTopP of candle-transformers
 * 0.8 [UPSTREAM-RECALLED: restated from memory of upstream, not from a copy]), evaluated on the device inside the same decode loop.
 * prs = softmax(logits / temperature) exactly as above.  The indices are ordered by prs descending, the LOWER index first among
 * equal values (candle's stable sort_by(total_cmp)); a prefix of that order is kept, the rest get probability 0, and the draw is
 * the multinomial above over the masked vector in vocabulary order (zeros included in the left-to-right fp32 cumulative weights).
 *   top_p  0 < top_p < 1, compared as (float)top_p: walk the order with a sequential fp32 running sum from 0; an element is kept
 *          while the sum BEFORE it is < top_p, so the prefix is the shortest whose sum is >= top_p (all of V if none is).
 *          top_p <= 0 or >= 1: off (Sampling::All), as in candle.  NaN: FL_ERR_BAD_ARGUMENT.
 *   top_k  0 < top_k < V: the first top_k of the order.  candle picks its k largest with select_nth_unstable_by and draws over
 *          them in that unspecified order, so which token a given random word maps to is not defined upstream; HERE it is: the
 *          masked form above.  The distribution is candle's.  top_k == 0 or >= V: off.  Negative: FL_ERR_BAD_ARGUMENT.
 *   both   the prefix is min(top_k, what top_p keeps): candle's TopKThenTopP.
 * Ties: temperature < 1e-7 stays ArgMax whatever top_p / top_k say, and ArgMax keeps the LAST maximal index; top_k = 1 keeps
 * the LOWEST maximal index (the stable order above).  The two differ on exact ties of the maximum, as they do in candle.
 * struct_size must be sizeof(fl_sampler) (FL_ERR_BAD_ARGUMENT otherwise); _reserved is 0. */
typedef struct fl_sampler {
    uint32_t struct_size;
    int32_t  top_k;
    double   temperature;
    double   top_p;
    uint64_t seed;
    uint64_t draws_done;
    int64_t  _reserved[2];
} fl_sampler;
int fl_forward_sample_ex(fl_model *m, fl_cache *c, const uint32_t *ids, size_t T, size_t pos,
                         const fl_sampler *sampler, uint32_t *token_out);
int fl_decode_sample_ex(fl_model *m, fl_cache *c, uint32_t first_token, size_t pos, size_t n_steps, int64_t eos,
                        const fl_sampler *sampler, uint32_t *tokens_out, size_t *n_out);

/* ---- speculative greedy decode: a multi-token verify step, cache rollback, prompt-lookup drafts ----------------------------------
 * New capability (the reference decodes one token per forward, mod.rs:411-453).  A decode step is bound by the read of the weights;
 * a forward over a few positions reads them once.  fl_forward_verify scores a drafted continuation in ONE forward and keeps the
 * longest prefix the model itself would have produced, so the output is still the model's own greedy output.
 *
 * GUARANTEE: every token these calls emit is the ArgMax (ties -> LAST maximal index, as fl_forward_argmax) of this library's forward
 * of the preceding tokens -- evaluated as a ROW OF A MULTI-ROW CALL (the prompt kernels), not as a one-row call (the decode kernels).
 * In bf16 the two paths can separate on a near-tie of the two largest logits, as the batch paths already can; nothing else may
 * separate them.  A model with FL_WEIGHTS_E4M3_ROW is accepted: its T > 1 rows run on the bf16 image of the same weights, as its
 * prompts do (and its n_draft == 0 steps on the FP8 stream, as its decode steps do). */
#define FL_VERIFY_MAX_DRAFT 15          /* T = n_draft + 1 <= 16: the last length before the short-prompt kernels' next tile step */

/* The cache forgets everything from position `len` on; the next call appends at `len`.  len > fl_cache_len(c):
 * FL_ERR_BAD_ARGUMENT.  A host-side length change (every call writes the device step state from it, and fl_batch_* reads it at the
 * start of each call, so it also works on a batch member between calls); a captured decode graph stays valid, and the cache's layout
 * choices, made from its capacity, do not change.  K/V rows beyond `len` stay in memory and are overwritten by the next append;
 * nothing reads past the length. */
int fl_cache_truncate(fl_cache *c, size_t len);

/* ---- K/V reuse across caches ----------------------------------------------------------------------------------------------------
 * New capability (the reference takes a fresh cache per request, mod.rs:370, and prefills the whole conversation again on every turn).
 * dst forgets what it holds and takes the first n cached positions of src (every layer, kv head and local shard); afterwards
 * fl_cache_len(dst) == n and the next call appends at n, exactly as if dst had computed those positions itself.  src is unchanged.
 * GUARANTEE: after fl_cache_copy_prefix(dst, src, n) any call on dst gives what the same call gives on src truncated to n -- bit for
 * bit when the two capacities are equal; when they differ the decode attention splits the keys differently (fl_cache_create picks the
 * split count from the capacity), and the results agree as those kernel variants agree among themselves.
 * The length is a host-side change, as in fl_cache_truncate: dst's captured decode graph stays valid, its layout choices (made from
 * its capacity) do not change, and it works on a batch member between two fl_batch_* calls.  The copy is ONE kernel launch per local
 * shard (k_kvcopy.hip), enqueued under the model's lock on the shard's stream: behind everything already submitted for either cache,
 * ahead of everything submitted later; the call does not wait for it (fl_cache_destroy of src does).  Any tp_mode: the copy is local to
 * each shard, and every rank of an FL_TP_MULTI_PROCESS group makes the same call.
 *   n == 0: fl_cache_reset(dst).  src == dst: fl_cache_truncate(dst, n).
 *   FL_ERR_BAD_ARGUMENT: a null cache, caches of different models, n > fl_cache_len(src).  FL_ERR_SEQ_OVERFLOW: n > fl_cache_capacity(dst).
 *   FL_ERR_UNSUPPORTED: the caches keep V in different layouts (FL_ATTN_MFMA changed between the two fl_cache_create calls).
 * All of these are decided before the device is touched. */
int fl_cache_copy_prefix(fl_cache *dst, const fl_cache *src, size_t n);

/* One forward of the T = n_draft + 1 ids [token, draft[0..n_draft)] at RoPE offset pos, appended at fl_cache_len with the mask of a
 * single fl_forward call of those ids.  a[t] = ArgMax of row t's logits; n_acc = the largest j <= n_draft with draft[i] == a[i] for
 * all i < j; tokens_out[0..n_acc] = a[0..n_acc] (the accepted drafts, then the model's own next token); *n_out = n_acc + 1.
 * Afterwards the cache length is L + n_acc + 1: `token` and the accepted drafts are cached, tokens_out[n_acc] is not -- it is the
 * `token` of the next call at pos + *n_out, exactly as fl_decode_greedy hands its last token on.  n_draft == 0 is the T = 1 decode
 * step (its mask, its kernels).  logits_out (host, or NULL) receives all T rows.  Never split into prefill chunks.
 * FL_ERR_BAD_ARGUMENT (before the device is touched): n_draft > FL_VERIFY_MAX_DRAFT, null tokens_out / n_out, an id >= vocab_size.
 * FL_ERR_UNSUPPORTED: tp_size > 1 (any mode); n_draft > the resolved sliding_window of a Mistral / Qwen2 model -- a decode step sees
 * the whole cache (no mask at T = 1) while a T-row call hides new key j from query t when j + window < t, so the rows equal
 * successive decode steps only while n_draft <= window.  Capacity and position overflow: as for a forward of T ids. */
int fl_forward_verify(fl_model *m, fl_cache *c, uint32_t token, const uint32_t *draft, size_t n_draft, size_t pos,
                      uint32_t *tokens_out /* [n_draft + 1] */, size_t *n_out, float *logits_out /* [n_draft + 1][V] host, or NULL */);

/* Prompt-lookup drafting: the continuation that followed the most recent earlier occurrence of the current n-gram. */
typedef struct fl_lookup {
    uint32_t struct_size;               /* sizeof(fl_lookup) */
    int32_t  max_draft;                 /* 0 .. FL_VERIFY_MAX_DRAFT; 0 = plain greedy steps */
    int32_t  ngram_max, ngram_min;      /* 1 <= ngram_min <= ngram_max <= 8 */
    int32_t  _pad;
    int64_t  _reserved[2];              /* 0 */
} fl_lookup;
typedef struct fl_spec_stats { uint64_t steps, drafted, accepted; } fl_spec_stats;

/* Pure host function, no GPU (like fl_tp_slice).  For n = ngram_max down to ngram_min, with n < n_history: the pattern is the last n
 * ids of history; s = the largest start with s + n < n_history and history[s .. s+n) == pattern (the most recent earlier occurrence
 * that has at least one id after it); the draft is history[s+n ..], cut to min(max_draft, limit) ids and to the end of history.  The
 * first n that matches wins.  No match, max_draft == 0 or limit == 0: *n_draft_out = 0.  A wrong struct_size, a range error in the
 * options, or null pointers: FL_ERR_BAD_ARGUMENT. */
int fl_lookup_draft(const uint32_t *history, size_t n_history, const fl_lookup *opts, size_t limit,
                    uint32_t *draft_out /* [limit] */, size_t *n_draft_out);

/* The loop of fl_decode_greedy (ArgMax only), built from verify steps: history = corpus ++ [first_token] ++ the tokens emitted so
 * far (the corpus is only the search text: normally the prompt, but it need not be what the cache holds); each step drafts with
 * limit = min(n_steps - emitted - 1, capacity left - 1, max_pos left - 1, sliding_window), verifies, and appends what the step
 * returned.  EOS as in fl_decode_greedy: the loop stops at the first emitted token == eos, that token is not written, later tokens
 * of the same step are dropped and the cache keeps the length fl_decode_greedy leaves.  Needs the room fl_decode_greedy needs and
 * never more.  One host synchronisation per step.  stats (or NULL): verify steps, drafted ids, accepted ids. */
int fl_decode_lookup(fl_model *m, fl_cache *c, const uint32_t *corpus, size_t n_corpus, uint32_t first_token, size_t pos,
                     size_t n_steps, int64_t eos, const fl_lookup *opts, uint32_t *tokens_out, size_t *n_out, fl_spec_stats *stats /* or NULL */);

/* ---- the same two calls for a SAMPLED request: exact multi-row verify ------------------------------------------------------------
 * The sampler of fl_forward_sample_ex is a pure function of (logits row, settings, index of the word of the seeded stream), and a
 * prompt-lookup draft is deterministic, so "accept draft d with probability p(d)" is the event "the draw of this row, with this row's
 * word, is d".  A sampled verify step draws row i with word sampler->draws_done + i (one more launch of the selection kernel's own
 * code, a workgroup per row) and keeps the longest prefix where the draws equal the drafts: acceptance is what rejection sampling
 * gives for a deterministic draft, and the output is the seeded stream of the plain loop -- token k is drawn with word k.
 *   sampler == NULL or temperature < 1e-7: the call IS fl_forward_verify / fl_decode_lookup, with the same launches.
 *   words: after a verify call the request has consumed *n_out words; the next call passes draws_done + *n_out.  Words of rejected
 *          rows are not consumed.  The library keeps no counter: every call brings draws_done, as it brings pos.
 *   n_draft == 0: the one-row sampled decode step (fl_forward_sample_ex of [token]): its kernels, bit for bit.
 *   fl_decode_lookup_ex is the loop of fl_decode_sample_ex: the EOS rule of fl_decode_lookup (the EOS token is not written, later
 *          tokens of that step are dropped, the cache keeps the length the plain loop leaves); it consumes the same words -- one per
 *          emitted token, plus the one that drew EOS -- and needs the same room and never more.  With max_draft == 0 it is
 *          fl_decode_sample_ex, bit for bit.
 * GUARANTEE: every emitted token is this library's sampler applied to this library's logits of the preceding tokens -- evaluated as
 * a ROW OF A MULTI-ROW CALL -- with the word the plain loop would use.  Logits of a multi-row call and of a one-row call differ in
 * the last bits (more so in bf16), and a draw that lands that close to a boundary of its cumulative interval can come out
 * differently in the two loops: the sampled form of the greedy step's near-tie sentence.  Nothing else may separate them.
 * Refusals: those of the greedy calls (tensor parallelism, n_draft > sliding_window, a cache with logit rules or a guide, sizes and
 * null pointers) plus the sampler's (a wrong struct_size, a NaN top_p, a negative top_k: FL_ERR_BAD_ARGUMENT), all decided before
 * the device is touched.  Logit rules, guides and log-probs inside verify steps: fl_forward_verify_lp / fl_decode_lookup_lp below.
 * Not built: tensor parallelism. */
int fl_forward_verify_ex(fl_model *m, fl_cache *c, uint32_t token, const uint32_t *draft, size_t n_draft, size_t pos,
                         const fl_sampler *sampler /* or NULL */, uint32_t *tokens_out /* [n_draft + 1] */, size_t *n_out,
                         float *logits_out /* [n_draft + 1][V] host, or NULL */);
int fl_decode_lookup_ex(fl_model *m, fl_cache *c, const uint32_t *corpus, size_t n_corpus, uint32_t first_token, size_t pos,
                        size_t n_steps, int64_t eos, const fl_lookup *opts, const fl_sampler *sampler /* or NULL */,
                        uint32_t *tokens_out, size_t *n_out, fl_spec_stats *stats /* or NULL */);

/* ---- packed verify: the verify steps of n <= 64 streams in ONE forward ------------------------------------------------------------
 * New capability: fl_forward_verify{,_ex} take one cache and read the weights once per stream; here the rows of every member's step
 * are the rows of one packed forward (fl_batch_prefill's: member i is appended to its own cache at its own RoPE offset, the cached
 * prefix unmasked, its new rows causal among themselves -- the mask of a verify step), the final norm and lm_head run on ALL rows in
 * blocks of FL_SCORE_ROWS rows (fl_tune "score_rows"; a last block of one row is avoided where the switch is 3 or more: the block
 * before it gives up a row), and one selection launch behind each block selects every row as its member's sampler says and scans
 * every member's drafts (k_verify_packed.hip).
 * Member i owns ids[offsets[i] .. offsets[i+1]) = [token, draft[0 .. n_draft_i)], n_draft_i <= FL_VERIFY_MAX_DRAFT.  Per member the
 * result is that of fl_forward_verify_ex(m, caches[i], token, draft, n_draft_i, pos[i], &samplers[i], ..) in the sense of its
 * GUARANTEE: every returned id is ArgMax, or this library's sampler with word draws_done_i + row, applied to this library's logits of
 * the preceding ids evaluated as a row of a multi-row call; tokens_out[offsets[i] ..] holds a[0 .. n_acc_i], n_out[i] = n_acc_i + 1,
 * the cache length becomes L_i + n_acc_i + 1, rejected rows' K/V stay behind the length.  Two differences: a member with n_draft_i == 0
 * is a row of this packed forward, not the one-row decode step; EOS is not interpreted (as in the single call).
 * WHAT A MEMBER'S RESULT DEPENDS ON.  Attention, RoPE and the K/V append see a member's own cache only.  The projections and lm_head
 * are planned by ROW COUNT -- the pack's total rows, and for lm_head the block's -- and the planner changes kernel or K slicing (i.e.
 * the fp32 summation order) at several counts: 1 -> 2, 32 -> 33 (wide gate/up), 128 -> 129, 256 / 512 / 768 .. in bf16, 64 -> 65 in
 * fp32.  So: among packs, and among score_rows values, that the planner serves with the same kernels and K split, a member's ids,
 * logits and cache contents are bit-identical wherever it sits and whoever its neighbours are; across such a threshold they are equal
 * up to fp32 summation order -- logits differ in the last bits, and at a near-tie of the two largest (more often in bf16) so can an
 * id: the GUARANTEE's sentence, nothing more.  Two thresholds are taken out: a pack of ONE row is forwarded as the row and a copy of
 * it (a stream left alone in a batcher equals the same stream among a few others), and fp32 models keep lm_head blocks within the
 * 2 .. 64 rows of one kernel (blocks capped at 64 rows, no one-row tail), so that there the score_rows switch changes nothing.
 * samplers NULL: ArgMax for all; one pack may mix ArgMax and sampled members.  logits_out (or NULL): the raw rows in pack order,
 * diagnostic -- one copy per block.  One host synchronisation per call; the ids and counts come back in one copy.
 * Memory: the [FL_SCORE_ROWS][V] fp32 block scratch is the scoring calls' (allocated at whichever call comes first, counted in
 * hbm_bytes_allocated: 33 MB at V = 32 000, 156 MB at V = 152 064 with the default 256 rows); a model's first SAMPLED packed verify
 * allocates a probability scratch of the same size (another 33 MB / 156 MB).
 * Refusals, all decided before the device or any cache is touched (a refused call modifies nothing; *n_out is zeroed):
 *   FL_ERR_BAD_ARGUMENT  those of fl_batch_prefill (nulls, n outside 1..64, offsets[0] != 0 or an empty member, the same cache twice,
 *                        a cache of another model, an id outside the vocabulary); a member with more than FL_VERIFY_MAX_DRAFT + 1
 *                        rows; a sampler error (struct_size, a NaN top_p, a negative top_k); null tokens_out / n_out
 *   FL_ERR_SEQ_OVERFLOW  per member, as fl_forward
 *   FL_ERR_UNSUPPORTED   tp_size > 1; n_draft_i above the sliding window of a Mistral / Qwen2 model; a member with logit rules or a guide
 * Not built: rules, guides and log-probs inside a packed verify, tensor parallelism, capturing the packed step in a graph. */
int fl_batch_verify(fl_model *m, fl_cache *const *caches, size_t n, const uint32_t *ids, const size_t *offsets /* [n+1] */,
                    const size_t *pos /* [n] */, const fl_sampler *samplers /* [n] or NULL: ArgMax for all */,
                    uint32_t *tokens_out /* [offsets[n]]: member i's ids at offsets[i] .. */, size_t *n_out /* [n] */,
                    float *logits_out /* [offsets[n]][V] or NULL, diagnostic, the raw rows in pack order */);
/* The loop of fl_decode_lookup_ex for n streams, built from packed verify steps.  Member i: search text corpus[corpus_offsets[i] ..
 * corpus_offsets[i+1]), first_tokens[i] at RoPE offset pos[i], n_steps[i] tokens wanted, eos[i] (< 0: none; eos NULL: none for all),
 * samplers[i] (NULL: ArgMax for all).  Per member it is fl_decode_lookup_ex in the GUARANTEE sense: the same drafting rule with the
 * same limit, the same EOS rule (the EOS is not written, later ids of that step are dropped, the cache keeps the length the plain
 * loop leaves), the same words (token k is drawn with word draws_done_i + k), the same room.  Each iteration drafts for every
 * unfinished member, packs those members only and runs ONE fl_batch_verify step with one host synchronisation; a member that has
 * its n_steps or its EOS leaves the pack.  opts->max_draft == 0 is allowed: every step is then a pack of one-row members.
 * tokens_out: [n][max over i of n_steps[i]], row-major; n_out [n]; stats [n] or NULL.  Refusals: fl_batch_verify's and fl_lookup's. */
int fl_batch_decode_lookup(fl_model *m, fl_cache *const *caches, size_t n, const uint32_t *corpus, const size_t *corpus_offsets /* [n+1] */,
                           const uint32_t *first_tokens, const size_t *pos, const size_t *n_steps /* [n] */, const int64_t *eos /* [n] or NULL */,
                           const fl_lookup *opts, const fl_sampler *samplers /* [n] or NULL */,
                           uint32_t *tokens_out /* [n][max n_steps] */, size_t *n_out /* [n] */, fl_spec_stats *stats /* [n] or NULL */);

/* Batched decode: B <= 64 caches of one model advanced together, one read of the weights per step for all
 * of them.  New capability: the reference runs concurrent streams as independent single-sequence loops
 * (mod.rs:137-238), each paying for the whole weight stream.  Every sequence keeps its own cache, RoPE
 * position and sampler state; per sequence the results are those of the single-sequence entry points
 * (same kernels' arithmetic, up to fp32 summation order in the norm).  bf16 or fp32 (fp32, and bf16 caches outside the MFMA attention
 * layout: RoPE and attention run per sequence, the projections once for all rows); one GPU, or -- bf16 -- the ranks of an FL_TP_MULTI_PROCESS group
 * with connected inboxes -- every rank then builds the same batch over its own caches and calls the same entry points in the same
 * order (the step's all-reduces and the gather of the ranks' logits blocks are collectives; a rank that stays away is
 * FL_ERR_RCCL after FL_AR_TIMEOUT_MS on the others).
 * The caches stay usable on their own (prefill them with fl_forward*, then batch the decode). */
typedef struct fl_batch fl_batch;
int  fl_batch_create(fl_model *m, fl_cache *const *caches, size_t n, fl_batch **out);
void fl_batch_destroy(fl_batch *b);
/* Continuous batching: `cache` (prefilled by fl_forward*, of the same model, not in the batch yet) takes the place of sequence
 * `slot` -- a stream that hit its EOS leaves, a waiting one joins -- without rebuilding the batch: one small copy, the step's captured
 * graph stays valid.  The cache that leaves is untouched and stays usable on its own.  A slot with no stream to serve can hold a
 * spare cache (its row is computed and ignored).  Not on a tensor-parallel group's batch while a step is outstanding on a peer:
 * every rank replaces the same slot between the same two steps.  (mod.rs:137-238: streams come and go independently.) */
int  fl_batch_replace(fl_batch *b, size_t slot, fl_cache *cache);
/* one step: tokens[i] at RoPE offset pos[i]; logits_out [n][V] fp32 host or NULL; argmax_out [n] or NULL */
int  fl_batch_forward(fl_batch *b, const uint32_t *tokens, const size_t *pos, float *logits_out, uint32_t *argmax_out);
/* the loop of fl_decode_greedy / fl_decode_sample for every sequence: tokens_out [n][n_steps], n_out [n];
 * a sequence stops counting at its EOS (its cache length is that of fl_decode_greedy); sampling may be NULL
 * (ArgMax); with sampling every sequence draws from its own copy of the seeded stream, as every request of
 * the reference does (seed 0 per request, mod.rs:373-374) */
int  fl_batch_decode(fl_batch *b, const uint32_t *first_tokens, const size_t *pos, size_t n_steps, int64_t eos,
                     const fl_sampling *sampling, uint32_t *tokens_out, size_t *n_out);
/* ... with every sequence's own EOS id (eos[i] < 0: none; eos NULL: none for all) and its own sampler (sampling[i]: temperature < 1e-7
 * is ArgMax; sampling NULL: ArgMax for all) -- a request's temperature is its own (chat.rs:24-25), and one batch serves requests that
 * differ in it.  draws_done lets a request span several calls, as in fl_decode_sample. */
int  fl_batch_decode_each(fl_batch *b, const uint32_t *first_tokens, const size_t *pos, size_t n_steps, const int64_t *eos,
                          const fl_sampling *sampling, uint32_t *tokens_out, size_t *n_out);

/* ... with an fl_sampler per sequence (samplers[i]; NULL: ArgMax for all): one batch mixes ArgMax, Sampling::All and top-p / top-k requests */
int  fl_batch_decode_each_ex(fl_batch *b, const uint32_t *first_tokens, const size_t *pos, size_t n_steps, const int64_t *eos,
                             const fl_sampler *samplers, uint32_t *tokens_out, size_t *n_out);

/* Packed prefill: n <= 64 prompts of one model in ONE forward.  New capability: the reference (and fl_forward*) forwards every
 * prompt on its own, and up to about 128 tokens a prompt's projections are a weight stream -- n short prompts read the weights n times.
 * Sequence i owns ids[offsets[i] .. offsets[i+1]) (at least one id), is appended to
 * caches[i] at its cached length, with RoPE offset pos[i] for its first id.  Per sequence the result is that of
 * fl_forward_sample_ex(m, caches[i], its ids, its count, pos[i], &samplers[i], &tokens_out[i]): the cache contents and length,
 * the sampler state (one draw), the token; logits_out [n][V] fp32 or NULL is what fl_forward would have returned for it.
 * samplers NULL: ArgMax for all.  The mask is fl_forward's, per sequence: the keys a cache held before the call are an unmasked
 * prefix, the causal and sliding-window mask runs over the sequence's own new tokens.  bf16 and fp32 models; caches in either layout,
 * also mixed (members outside the MFMA attention layout: attention per sequence, the projections still once for all rows).
 * FL_ERR_BAD_ARGUMENT, before the device or any cache is touched: a null m / caches / ids / offsets / pos, n == 0 or n > 64,
 * offsets[0] != 0 or offsets that do not increase (an empty sequence), the same cache twice, a cache of another model, an id outside
 * the vocabulary.  FL_ERR_SEQ_OVERFLOW per sequence as fl_forward.  FL_ERR_UNSUPPORTED: tp_size > 1 in any mode; more than
 * FL_PREFILL_CHUNK (8192) tokens in all -- the caller splits, this call never chunks.  A refused call modifies nothing: no cache
 * length, no sampler state. */
int fl_batch_prefill(fl_model *m, fl_cache *const *caches, size_t n, const uint32_t *ids, const size_t *offsets /* [n+1] */,
                     const size_t *pos /* [n] */, const fl_sampler *samplers /* [n] or NULL */,
                     uint32_t *tokens_out /* [n] or NULL */, float *logits_out /* [n][V] or NULL */);

/* ---- token log-probabilities: the chosen token's, and the N most likely tokens', inside the device decode loop ------------------
 * New capability (the reference reports none).  What an OpenAI-compatible server is asked for as `logprobs` / `top_logprobs`.  The
 * values are computed by one more launch behind each step's token selection, inside the same replayed graph; per step 4 + 160 bytes
 * come back with the token ids at the end of a chunk.  A call without log-probs launches exactly what it launched before.
 *
 * For a step whose fp32 logits row is x[0..V) (what fl_forward returns for that step), m = max_j x[j]:
 *     lp[i] = (x[i] - m) - log(sum_j exp(x[j] - m))                      (natural log)
 * THE DISTRIBUTION IS THE MODEL'S OWN: temperature 1, no top-p / top-k mask.  It does not depend on the sampler that chose the token:
 * a greedy request and a temperature = 0.7, top_p = 0.9 request report the same lp for the same row.
 *   token_logprob[s] = lp[token s], the id the step's selection produced (ArgMax or sampled).
 *   top_ids[s][0..top_n), top_logprobs[s][..]: the first top_n ids of the order "logit descending, LOWER index first among equal
 *       values" (the stable order of fl_sampler above), each with its lp.  ArgMax keeps the LAST maximal index, so on an exact tie of
 *       the maximum the chosen token can differ from top_ids[s][0], as it does between ArgMax and top_k = 1.
 * Arithmetic: x[j] - m in fp32, precise expf, the sum in fp64, then log and the final subtraction.  -inf entries contribute 0 and have
 * lp = -inf.  A row without a finite maximum, or with NaN, gives unspecified values (never a fault; every reported id is < V).
 * EOS as in fl_decode_*: the EOS token is not emitted; only entries [0, *n_out) of the arrays are defined.
 * The tokens, the cache state and the sampler's draw count after an _lp call are exactly those of the matching _ex call.
 * FL_ERR_BAD_ARGUMENT (before the device is probed): null lp, wrong struct_size, top_n outside 0 .. FL_LOGPROBS_MAX_TOP or above the
 * vocabulary, a missing array, nonzero _reserved.  FL_ERR_UNSUPPORTED (before the device is touched): tp_size > 1 in any mode, a
 * batch on a tensor-parallel group.  Any dtype and weight format otherwise.
 * Memory: a cache's FIRST log-prob call allocates its record buffer (4096 records of 164 bytes, 656 KB of HBM, freed with the cache);
 * the model's first one 656 KB of pinned host memory.  Caches that never ask pay nothing. */
#define FL_LOGPROBS_MAX_TOP 20
typedef struct fl_logprobs {
    uint32_t  struct_size;      /* sizeof(fl_logprobs), FL_ERR_BAD_ARGUMENT otherwise */
    int32_t   top_n;            /* 0 .. FL_LOGPROBS_MAX_TOP */
    float    *token_logprob;    /* host [n]            : required */
    uint32_t *top_ids;          /* host [n][top_n]     : required iff top_n > 0 */
    float    *top_logprobs;     /* host [n][top_n]     : required iff top_n > 0 */
    int64_t   _reserved[2];     /* 0 */
} fl_logprobs;
/* fl_forward_sample_ex / fl_decode_sample_ex / fl_batch_decode_each_ex with log-probs.  sampler(s) NULL: ArgMax.
 * n = 1 / n_steps / n_steps rows per sequence (lp[i] is sequence i's, with its own top_n and arrays). */
int fl_forward_sample_lp(fl_model *m, fl_cache *c, const uint32_t *ids, size_t T, size_t pos, const fl_sampler *sampler,
                         uint32_t *token_out, const fl_logprobs *lp);
int fl_decode_sample_lp(fl_model *m, fl_cache *c, uint32_t first_token, size_t pos, size_t n_steps, int64_t eos,
                        const fl_sampler *sampler, uint32_t *tokens_out, size_t *n_out, const fl_logprobs *lp);
int fl_batch_decode_each_lp(fl_batch *b, const uint32_t *first_tokens, const size_t *pos, size_t n_steps, const int64_t *eos,
                            const fl_sampler *samplers, uint32_t *tokens_out, size_t *n_out, const fl_logprobs *lp /* [n_seq] */);

/* ---- prompt log-probabilities: every row of a forward scored on the device ---------------------------------------------------------
 * New capability (the reference reports none).  What an OpenAI-compatible server is asked for as `echo` + `logprobs`, the open-source
 * servers as `prompt_logprobs`, an evaluation harness as `loglikelihood`: the log-probability of tokens the model did NOT generate.
 * fl_forward_score is fl_forward with every row scored: the cache ends up exactly as fl_forward leaves it (the same chunks of
 * FL_PREFILL_CHUNK, the same mask, the same per-layer launches; T = 1 takes the decode step), but behind each chunk's layers the final
 * norm runs on all its rows, lm_head runs in blocks of FL_SCORE_ROWS rows (default 256; fl_tune "score_rows", 1 .. 1024) into one
 * [rows][V] fp32 scratch, and each block is followed by one launch that scores its rows.  T x V logits never exist at once; per row
 * 168 bytes come back, in one copy per call.  No token is selected.  Logit rules and a guide installed on the cache are neither
 * applied nor counted: THE DISTRIBUTION IS THE MODEL'S OWN, as for fl_logprobs.
 *
 * Row t (the position of ids[t]) has the fp32 logits x[0..V) that a prefill of ids[0 .. t] would return, and lp as defined for
 * fl_logprobs above -- the same arithmetic (x[j] - m in fp32, precise expf, the sum in fp64, then log and the final fp32 subtraction),
 * the same kernel code.  Its target is targets[t]; targets == NULL means next-token scoring: row t's target is ids[t + 1] and the
 * last row has none.  FL_SCORE_NO_TARGET: the row has none.
 *   target_logprob[t] = lp[target]; a quiet NaN where the row has no target.
 *   target_rank[t]    = 1 + the number of ids that precede the target in the order "logit descending, LOWER index first among equal
 *                       values" (so: 1 = it is top_ids[t][0]; whenever rank <= top_n, top_ids[t][rank - 1] == target); 0 where the row
 *                       has no target.  Defined for a -inf target too.
 *   top_ids[t][0..top_n), top_logprobs[t][..]: as for fl_logprobs, reported whether or not the row has a target.
 * A row with NaN, or without a finite maximum, gives unspecified values (never a fault; every reported id is < V).
 * logits_out (or NULL): host [T][V], the rows the scoring kernel read -- a DIAGNOSTIC like fl_forward_verify's (T x V x 4 bytes cross
 * the bus): for tests and tools, not for production use.
 * fl_batch_score is fl_batch_prefill (without tokens_out) with every row scored: the same checks and limits, the same layers, the
 * caches as it leaves them; ONE fl_score whose arrays run over all offsets[n] rows; with targets == NULL the shift is per sequence
 * (the last row of every member has no target).
 * FL_ERR_BAD_ARGUMENT, before the device or a cache is touched, naming the field: null sc, wrong struct_size, top_n outside
 * 0 .. FL_LOGPROBS_MAX_TOP or above the vocabulary, a missing required array, a target >= V other than FL_SCORE_NO_TARGET, nonzero
 * _reserved; then the errors of fl_forward / fl_batch_prefill.  FL_ERR_UNSUPPORTED: tp_size > 1 in any mode.  Any dtype and weight
 * format otherwise.
 * Memory: a model's FIRST scoring call allocates the block scratch (FL_SCORE_ROWS x V x 4 bytes of HBM: 33 MB at V = 32 000, 156 MB at
 * V = 152 064 with the default 256) and the target / record buffers (172 bytes of HBM and of pinned host memory per row of the largest
 * call seen); they are counted in fl_model_hbm_bytes and freed with the model.  Models that never score pay nothing.
 * Not here: scoring under tensor parallelism, inside verify / lookup steps, echoed log-probs in StreamBatcher, prompt log-probs under
 * logit rules or a guide, a softmax reduction fused into the lm_head GEMM (no logits in memory at top_n = 0). */
#define FL_SCORE_NO_TARGET 4294967295u   /* 0xffffffff */
typedef struct fl_score {
    uint32_t  struct_size;      /* sizeof(fl_score), FL_ERR_BAD_ARGUMENT otherwise */
    int32_t   top_n;            /* 0 .. FL_LOGPROBS_MAX_TOP */
    const uint32_t *targets;    /* host [T] or NULL (next-token scoring); an entry is < V or FL_SCORE_NO_TARGET */
    float    *target_logprob;   /* host [T]            : required */
    uint32_t *target_rank;      /* host [T]            : optional */
    uint32_t *top_ids;          /* host [T][top_n]     : required iff top_n > 0 */
    float    *top_logprobs;     /* host [T][top_n]     : required iff top_n > 0 */
    float    *logits_out;       /* host [T][V]         : optional, diagnostic */
    int64_t   _reserved[2];     /* 0 */
} fl_score;
int fl_forward_score(fl_model *m, fl_cache *c, const uint32_t *ids, size_t T, size_t pos, const fl_score *sc);
int fl_batch_score(fl_model *m, fl_cache *const *caches, size_t n, const uint32_t *ids, const size_t *offsets /* [n+1] */,
                   const size_t *pos /* [n] */, const fl_score *sc /* ONE struct, arrays over offsets[n] rows */);

/* ---- decoder-model embeddings: pooled final hidden states of a packed forward, optionally under a full (bidirectional) mask ---------
 * The embedding checkpoints deployed today are decoder models of the three architectures this library runs: e5-mistral /
 * SFR-Embedding-Mistral / Linq-Embed-Mistral (causal, last-token pooling), gte-Qwen2 (full mask, last-token pooling), LLM2Vec-style
 * Llama (full mask, mean pooling); reward and *ForSequenceClassification heads need a row's final hidden state (FL_POOL_NONE, the
 * caller applies the head).  fl_batch_embed is fl_batch_prefill's pack -- 1..64 members, at most 8192 tokens, every member non-empty,
 * caches of this model, member i appended to caches[i] at RoPE offset pos[i] -- with a tail that pools instead of projecting: no
 * lm_head, no token selection.  Installed logit rules and guides are ignored and left alone (as by fl_forward).
 *   hidden state of row t: hid[t][j] = (x[t][j] * inv_rms[t]) * w[j], the model's final RMSNorm taken from the fp32 residual stream
 *                          (bf16 models too), each multiply rounded to fp32 on its own.
 *   pooling runs over the CALL's rows of a member only: a cached prefix (fl_cache_copy_prefix of a shared instruction) is attended
 *   to, not pooled.  LAST / FIRST: that row.  MEAN: the fp32 sum over the member's rows in row order (one rounded add per row, from
 *   +0), then one rounded division by (float)count.  NONE: every row, out is [offsets[n]][dims].
 *   dims = dimensions ? dimensions : hidden_size: the first dims columns are kept, THEN (normalize) out[j] = p[j] / sqrt(sum p[j]^2)
 *   in fp32; a zero vector stays zero.  The order of the sum of squares is fixed: the same call gives the same bits every time, and
 *   a member's vector does not depend on the rest of the pack beyond what fl_batch_prefill's rows do.
 *   out: host [n][dims] fp32 (LAST / MEAN / FIRST) or [offsets[n]][dims] (NONE; normalize applies per row).
 * FL_MASK_CAUSAL leaves every cache exactly as fl_batch_prefill of the same pack leaves it (contents and length): decoding may go on
 * from it.  FL_MASK_FULL: every row of a member sees all of the member's keys [0, len + count); the sliding window is not applied.
 * It needs EMPTY caches (a prefix computed causally is not the bidirectional model's).  Afterwards the cache length has advanced by
 * count as after a prefill, but its K/V are the full-mask model's: fl_cache_reset before decoding from or prefilling into it.
 * FL_ERR_BAD_ARGUMENT, before the device or a cache is touched: null pointers, wrong struct_size, nonzero _reserved, unknown
 * pooling / mask, normalize not 0 / 1, dimensions outside 0 .. hidden_size; then fl_batch_prefill's.  FL_ERR_UNSUPPORTED: tp_size > 1
 * in any mode, FL_MASK_FULL on a cache that is not empty.  Any dtype and weight format otherwise (FL_WEIGHTS_E4M3_ROW models run
 * prompts through the bf16 kernels).
 * Memory: a model's first embed call allocates max(n, offsets[n]) x hidden_size x 4 bytes of HBM (growing with the largest call,
 * half as much again each time, never more than a call can hold), counted in fl_model_hbm_bytes; models that never embed pay
 * nothing.
 * Not here: the tokenizer (and appending EOS for e5-style models), latent-attention pooling (NV-Embed), per-layer hidden states,
 * embeddings under tensor parallelism, FL_MASK_FULL over a cached prefix, a StreamBatcher lane for embedding requests, the pool fused
 * into the last down_proj epilogue. */
typedef enum fl_pooling   { FL_POOL_LAST = 0, FL_POOL_MEAN = 1, FL_POOL_FIRST = 2, FL_POOL_NONE = 3 } fl_pooling;
typedef enum fl_attn_mask { FL_MASK_CAUSAL = 0, FL_MASK_FULL = 1 } fl_attn_mask;
typedef struct fl_embed {
    uint32_t struct_size;   /* sizeof(fl_embed) */
    int32_t  pooling;       /* fl_pooling */
    int32_t  mask;          /* fl_attn_mask */
    int32_t  normalize;     /* 0 / 1: divide each output vector by its L2 norm */
    int64_t  dimensions;    /* 0: hidden_size; else 1..hidden_size: keep the first `dimensions` columns, THEN normalise
                               (OpenAI `dimensions`, Matryoshka checkpoints) */
    int64_t  _reserved[2];  /* 0 */
} fl_embed;
int fl_batch_embed(fl_model *m, fl_cache *const *caches, size_t n, const uint32_t *ids, const size_t *offsets /* [n+1] */,
                   const size_t *pos /* [n] */, const fl_embed *opts, float *out);

/* ---- logit rules: logit_bias and repetition / frequency / presence penalties inside the device decode loop -------------------------
 * New capability (the reference has none).  What an OpenAI-compatible server is asked for as `logit_bias`, `frequency_penalty`,
 * `presence_penalty`, and the `repetition_penalty` of the open-source servers.  The rules belong to a cache: installing them gives
 * the cache a table of V entries {word, bias} -- word bit 31 "the id occurred in the prompt", bits 0..30 c, the times the id was
 * produced as output -- that the decode step itself keeps up to date, by one more launch between lm_head and token selection inside
 * the same replayed graph.  A cache that never installs rules runs exactly what it ran before.
 *
 * For a step whose fp32 logits row is x[0..V) (what fl_forward returns for it) the selection sees y; every operation is rounded to
 * fp32 on its own, in this order, nothing contracted into an FMA (a numpy float32 restatement reproduces the bits):
 *     y = x[j]
 *     if word != 0 and repetition_penalty != 1:  y = (y > 0) ? y / rp : y * rp        (HF / vLLM form; y == 0 stays 0)
 *     if c > 0:                                  y = y - (float)c * frequency_penalty
 *                                                y = y - presence_penalty
 *     y = y + bias                                                        (0 for ids without one; -inf bans an id)
 * ArgMax (still the LAST maximal index), temperature, top-p and top-k then run on y exactly as they run on x without rules.
 * Counting: the install seeds the table -- prompt_ids set bit 31, output_ids are counted.  Afterwards fl_decode_* and
 * fl_batch_decode* count the INPUT token of every step as one more output before that step's row is adjusted (a decode step's input
 * is the previous step's output, also across chunks and calls): at the step that produces output s the table holds outputs 0..s-1,
 * each once.  fl_forward_* calls (any T) count nothing: their ids are prompt, which the seed covers.  After a decode call that
 * stopped at its EOS the table is unspecified until the next install (the steps behind the EOS ran and were discarded).
 * Log-probs (fl_*_lp) keep reporting the model's own distribution from the raw row; fl_forward / fl_batch_forward logits stay raw.
 * Honoured by fl_forward_argmax, fl_forward_sample{,_ex,_lp}, fl_decode_greedy, fl_decode_sample{,_ex,_lp}, fl_batch_decode,
 * fl_batch_decode_each{,_ex,_lp}.  FL_ERR_UNSUPPORTED, before the device or any cache is touched, while a cache involved has rules:
 * fl_forward_verify, fl_decode_lookup, fl_batch_prefill with tokens_out, fl_batch_forward with argmax_out; and the install itself on
 * a model with tp_size > 1.  fl_cache_truncate, fl_cache_copy_prefix and fl_cache_reset leave the rules and the table alone: a caller
 * that rolls a request back installs again.
 * FL_ERR_BAD_ARGUMENT, before the device is probed and with the cache as it was: wrong struct_size, nonzero _reserved, a NaN or
 * out-of-range scalar, an id >= V in any list, n_bias > V or a duplicate bias id, a null list with a nonzero count.
 * Memory: a cache's first install allocates V x 12 bytes of HBM + a control block (1.8 MB at V = 152 064) and V x 8 bytes of pinned
 * host memory, freed with the cache; a batch's first step with a ruled member B x V x 4 bytes. */
typedef struct fl_logit_rules {
    uint32_t        struct_size;          /* sizeof(fl_logit_rules), FL_ERR_BAD_ARGUMENT otherwise */
    uint32_t        n_bias;               /* 0 .. V entries below, ids distinct */
    const uint32_t *bias_ids;             /* [n_bias] */
    const float    *bias_values;          /* [n_bias] not NaN, not +inf; -inf allowed */
    float           repetition_penalty;   /* finite, > 0; 1: off */
    float           frequency_penalty;    /* finite; 0: off */
    float           presence_penalty;     /* finite; 0: off */
    int64_t         _reserved[2];         /* 0 */
} fl_logit_rules;
/* rules NULL: remove (the lists are ignored; the cache runs its old graphs again).  Otherwise install: the table is built on the host
 * and sent with one asynchronous copy on the model's stream, ahead of whatever is submitted next. */
int fl_cache_set_logit_rules(fl_model *m, fl_cache *c, const fl_logit_rules *rules, const uint32_t *prompt_ids, size_t n_prompt,
                             const uint32_t *output_ids, size_t n_output);
/* The table words [V] (bit 31: prompt, bits 0..30: output count) once the stream is idle.  FL_ERR_BAD_ARGUMENT: no rules installed. */
int fl_cache_logit_counts(fl_model *m, fl_cache *c, uint32_t *words_out);

/* ---- guided decoding: a token-level automaton inside the device decode loop ---------------------------------------------------------
 * New capability (the reference has none).  What an OpenAI-compatible server is asked for as `response_format` (JSON mode, JSON
 * schema), strict tool calls, regex or choice constraints: requests whose allowed tokens depend on what has been produced so far.
 * The library takes the constraint in the form the open-source servers hand to their GPUs, a finite automaton over token ids
 * (Outlines' index, vLLM's guided decoding); it needs no tokenizer and no grammar (fastllm_host.hpp has compile_guide, from a
 * byte-level DFA and a vocabulary).  An fl_guide is immutable, belongs to one model and may be installed in any number of its caches.
 *
 * The automaton is CSR: state s allows the ids tokens[row_ptr[s] .. row_ptr[s + 1]), and tokens[e] leads to state next[e].
 * While a guide is installed in a cache at state s, every call that selects a token on that cache selects from y:
 *     y[j] = x[j]   bit for bit, if j is in the list of s
 *     y[j] = -inf   otherwise
 * where x is the row the selection would otherwise have read: the raw fp32 logits, or the rule-adjusted row when logit rules are
 * installed too (rules first, mask last: a positive bias does not bring a disallowed id back).  The selected token t moves the cache
 * to next(s, t); a t without an edge (possible only for a row with NaN) leaves the state where it is.  One more launch between lm_head
 * and token selection inside the same replayed graph does both, the advance from the step's input token; a cache without a guide runs
 * exactly what it ran before.  The state of a guided cache is the state in which the NEXT selected token is looked up.
 * The host is authoritative for the state, as it is for the cached length: the library writes it to the device at the start of every
 * call and of every chunk of a decode call, the device advances it inside a chunk, and the host walks the tokens that came back (the
 * emitted ones, and the EOS if one ended the call) through its own copy.  Steps that ran behind an EOS are discarded for the state as
 * they are for the length.  fl_cache_truncate, fl_cache_reset and fl_cache_copy_prefix touch neither the guide nor the state: a
 * caller that rolls a request back sets the state again (fl_cache_set_guide with the same guide).
 * Honoured by fl_forward_argmax, fl_forward_sample{,_ex,_lp}, fl_decode_greedy, fl_decode_sample{,_ex,_lp}, fl_batch_decode,
 * fl_batch_decode_each{,_ex,_lp}.  Log-probs (fl_*_lp) keep reporting the model's own distribution from the raw row; fl_forward /
 * fl_batch_forward logits stay raw, and fl_forward (which selects nothing) leaves the state alone.
 * FL_ERR_UNSUPPORTED, before the device or any cache is touched: fl_guide_create and fl_cache_set_guide on a model with tp_size > 1
 * (any mode, so no member of a tensor-parallel batch can be guided); a guided cache in fl_forward_verify, fl_decode_lookup,
 * fl_batch_prefill with tokens_out, fl_batch_forward with argmax_out.
 * FL_ERR_BAD_ARGUMENT from fl_guide_create, before the device is probed: wrong struct_size, nonzero _reserved, n_states == 0, a null
 * array, row_ptr not starting at 0 or decreasing, a state without an edge (it would make every logit -inf), tokens not strictly
 * ascending within a state, an id >= V, a next >= n_states.  Creation validates all of that so that the kernel need not.
 * Memory: 8 bytes per edge + 8 per state, once in HBM and once on the host, per guide (an automaton over V = 152 064 with a few hundred
 * dense states is hundreds of MB: the known cost of this representation); per guided cache V x 4 bytes + a control block, per batch
 * with a guided member B x V x 4 bytes. */
typedef struct fl_guide fl_guide;
typedef struct fl_guide_desc {
    uint32_t        struct_size;          /* sizeof(fl_guide_desc), FL_ERR_BAD_ARGUMENT otherwise */
    uint32_t        n_states;             /* >= 1 */
    const uint64_t *row_ptr;              /* [n_states + 1] row_ptr[0] == 0, non-decreasing; nnz = row_ptr[n_states] */
    const uint32_t *tokens;               /* [nnz] strictly ascending within a state, < V */
    const uint32_t *next;                 /* [nnz] < n_states */
    int64_t         _reserved[2];         /* 0 */
} fl_guide_desc;
int  fl_guide_create(fl_model *m, const fl_guide_desc *desc, fl_guide **out);
/* Drops the creator's reference; a cache that has the guide installed holds one of its own and keeps working. */
void fl_guide_destroy(fl_guide *g);
/* Installs g at `state` (< n_states, FL_ERR_BAD_ARGUMENT otherwise), replacing whatever was installed; g NULL: removes the guide
 * (state is ignored; the cache runs its old graphs again). */
int  fl_cache_set_guide(fl_model *m, fl_cache *c, fl_guide *g, uint32_t state);
/* The state in which the next selected token is looked up.  FL_ERR_BAD_ARGUMENT: no guide installed. */
int  fl_cache_guide_state(const fl_cache *c, uint32_t *state_out);

/* ---- speculative decode for full requests: logit rules, guides and log-probs inside verify steps ------------------------------------
 * fl_forward_verify{,_ex} and fl_decode_lookup{,_ex} understand only a sampler and KEEP REFUSING a cache with logit rules or a guide.
 * These two calls are the superset: the same verify step and the same loop on a cache that may have rules, a guide or both, with
 * optional log-probs (the _lp convention: sampler NULL or temperature < 1e-7 is ArgMax, lp NULL reports nothing).  One launch between
 * lm_head and the step's selection (verify_adjust_kernel) writes the rows the selection reads; a cache with neither rules nor a guide
 * and lp == NULL runs exactly the launches of fl_forward_verify_ex.
 *   Counting.  Row i of a step sees the rules table that the plain ruled loop (fl_decode_sample_lp with the same rules) would hold at
 *     its step i: that loop counts each step's INPUT token before it adjusts the row, so row i is adjusted with the table after the
 *     inputs of rows 0..i -- token, draft[0..i).  The launch only reads the table; after the call the table has counted the inputs of
 *     rows 0..n_acc, the rows the call kept (one small launch behind the selection, ahead of everything submitted later).  In the loop
 *     an EOS at returned id i counts the inputs of rows 0..i only: what the plain loop holds when it draws that EOS.
 *   Guide.  Row i is masked in the state after draft[0..i); fl_cache_guide_state afterwards is the state after the ids the call
 *     returned, the EOS's edge included, as in the plain loop.  Rules first, mask last, as in the one-row step.
 *   Draft trimming.  A draft id with no edge from the state reached is -inf in the row before it and can never be accepted, so both
 *     calls cut the draft at the first such id before they forward: the returned ids do not change, logits_out holds one row per
 *     remaining id (+ 1), and stats.drafted counts the cut draft.  Bias and penalties do not cut drafts.
 *   Log-probs are the model's own distribution, computed from the RAW row of each returned id, whatever rules or guide chose it (as in
 *     fl_decode_sample_lp); entry k of lp's arrays belongs to the k-th returned / emitted id.  logits_out are the raw rows.
 *   n_draft == 0 (also after trimming), or a loop step without drafts: one step of fl_decode_sample_lp (counted, guided), bit for bit;
 *     on a cache with neither rules nor a guide and lp == NULL, the step fl_forward_verify_ex / fl_decode_lookup_ex take there.
 *   max_draft == 0: the loop IS fl_decode_sample_lp (on such a bare cache without lp: fl_decode_lookup_ex with max_draft == 0).
 * GUARANTEE: that of fl_forward_verify_ex -- every emitted token is this library's sampler applied to the rule-adjusted, guide-masked
 * logits of the preceding tokens, evaluated as a ROW OF A MULTI-ROW CALL, with the word the plain loop would use.  Logits of a
 * multi-row call and of a one-row call differ in the last bits (more so in bf16), and a choice that lands that close to a tie or to a
 * boundary of its cumulative interval can come out differently in the two loops.  Nothing else may separate them.
 * Refusals: those of the _ex calls (tensor parallelism, n_draft > sliding_window, sizes, null pointers, the sampler's argument errors)
 * plus those of fl_logprobs, all decided before the device is touched.  Not built: rules, guides and log-probs in a packed verify
 * (fl_batch_verify), tensor parallelism, capturing the step in a graph.
 * Memory: a model's first ruled or guided verify step allocates [16][V] fp32 of HBM (2 MB at V = 32 000, 9.7 MB at V = 152 064),
 * its first with log-probs 16 records; both are counted in fl_model_hbm_bytes and freed with the model. */
int fl_forward_verify_lp(fl_model *m, fl_cache *c, uint32_t token, const uint32_t *draft, size_t n_draft, size_t pos,
                         const fl_sampler *sampler /* or NULL */, const fl_logprobs *lp /* or NULL; arrays [n_draft + 1] */,
                         uint32_t *tokens_out /* [n_draft + 1] */, size_t *n_out, float *logits_out /* [n_draft + 1][V] raw rows, or NULL */);
int fl_decode_lookup_lp(fl_model *m, fl_cache *c, const uint32_t *corpus, size_t n_corpus, uint32_t first_token, size_t pos,
                        size_t n_steps, int64_t eos, const fl_lookup *opts, const fl_sampler *sampler /* or NULL */,
                        const fl_logprobs *lp /* or NULL; arrays [n_steps] */, uint32_t *tokens_out, size_t *n_out,
                        fl_spec_stats *stats /* or NULL */);

int fl_synchronize(fl_model *m);

/* ---- embeddings: the BERT / MiniLM encoder forward --------------------------------------------------------------------------------
 * The reference's second model path: trait EmbeddingModel (src/models/embeddings.rs:17-38), implemented by MiniLMModel on the CPU in
 * fp32, one text at a time (embeddings.rs:289).  Here the same forward runs on the GPU over a packed batch of sequences.
 * What is reproduced (line numbers of src/models/embeddings.rs):
 *   input    x = LayerNorm(word_embeddings[ids] + position_embeddings[0..T)), eps hard-wired to 1e-12 (:315-318); token-type embeddings
 *            are never added (:370-378) -- HF's BertModel adds row 0, which add_token_type0 = 1 restores.
 *   layer    post-LN (:130-243): a = softmax(Q K^T / sqrt(d)) V with NO mask (bidirectional; heads hidden_size / num_attention_heads
 *            wide, :77); x = LN(x + dense(a)); x = LN(x + output(gelu(intermediate(x)))); eps = layer_norm_eps (:104-109, :213-218).
 *   gelu     candle's Tensor::gelu (:229-231) is the TANH form 0.5 v (1 + tanh(sqrt(2/pi) v (1 + 0.044715 v^2))); gelu_erf is the exact
 *            one [UPSTREAM-RECALLED: restated from memory of upstream candle, not from a copy].  HF checkpoints of this family were
 *            trained with the erf form, so both are offered; the reference's is the default.
 *   LN       candle_nn::LayerNorm: mean and biased variance over hidden_size in fp32, (x - mean) / sqrt(var + eps) * w + b.
 *   pooling  the attention mask is all ones (:346-368): the mean of the last hidden states over the sequence's tokens (:430-433),
 *            divided by its L2 norm (:341-344, :436).
 * Tensor names carry no "bert." prefix (:298-327): embeddings.word_embeddings.weight [V,h], embeddings.position_embeddings.weight
 * [P,h], embeddings.LayerNorm.{weight,bias}, and per layer encoder.layer.{i}. attention.self.{query,key,value}.{weight,bias},
 * attention.output.dense.{weight,bias}, attention.output.LayerNorm.{weight,bias}, intermediate.dense.{weight,bias},
 * output.dense.{weight,bias}, output.LayerNorm.{weight,bias}; with add_token_type0 also embeddings.token_type_embeddings.weight [*,h].
 * One GPU; submission is serialised per encoder.  compute_dtype FL_DTYPE_F32 is the parity mode; in FL_DTYPE_BF16 the GEMM inputs,
 * Q / K / V, the attention probabilities and the GELU output are bf16, the residual stream and the LayerNorm statistics fp32.
 * fl_encoder_create, decided before the device probe: FL_ERR_BAD_CONFIG (a size that is not positive, heads that do not divide
 * hidden_size); FL_ERR_UNSUPPORTED (head_dim other than 32 or 64 -- so hidden_size is always a multiple of 8 --, intermediate_size not a multiple of 8);
 * FL_ERR_BAD_ARGUMENT (unknown activation, wrong struct_size, non-zero _pad / _reserved, null cfg / out, compute dtype other than F32 / BF16).  Afterwards:
 * FL_ERR_NO_DEVICE (there is no CPU path), FL_ERR_MISSING_TENSOR / FL_ERR_SHAPE_MISMATCH.
 * Per call, decided before any launch: FL_ERR_BAD_ARGUMENT (an empty sequence -- the reference would divide by zero --, offsets that
 * do not start at 0 or decrease, an id >= vocab_size, null pointers); FL_ERR_SEQ_OVERFLOW (a sequence longer than
 * max_position_embeddings, more than max_batch_tokens tokens in all).  The encoder stays usable after any of them. */
typedef enum fl_activation { FL_ACT_GELU_TANH = 0 /* the reference */, FL_ACT_GELU_ERF = 1 } fl_activation;
typedef struct fl_encoder_config {
    uint32_t struct_size;            /* sizeof(fl_encoder_config), else FL_ERR_BAD_ARGUMENT */
    int32_t  activation;             /* fl_activation */
    int32_t  add_token_type0;        /* 0: as the reference; 1: + embeddings.token_type_embeddings.weight[0] (HF) */
    int32_t  _pad;
    int64_t  hidden_size, intermediate_size, num_hidden_layers, num_attention_heads,
             max_position_embeddings, vocab_size;
    int64_t  max_batch_tokens;       /* workspace, allocated once at create; 0 -> 4096 */
    double   layer_norm_eps;
    int64_t  _reserved[2];           /* 0, else FL_ERR_BAD_ARGUMENT */
} fl_encoder_config;
typedef struct fl_encoder fl_encoder;
int  fl_encoder_create(const fl_encoder_config *cfg, const fl_tensor *tensors, size_t n_tensors,
                       int32_t compute_dtype /* FL_DTYPE_F32 | FL_DTYPE_BF16 */, int32_t device, fl_encoder **out);
void fl_encoder_release(fl_encoder *e);
/* last hidden states of ONE sequence, [T][h] fp32 host: what MiniLMModel::forward returns (embeddings.rs:380-393) */
int  fl_encoder_hidden(fl_encoder *e, const uint32_t *ids, size_t T, float *out);
/* n_seq sequences packed back to back: sequence s is ids[offsets[s] .. offsets[s+1]); out [n_seq][h] fp32 host =
 * L2-normalised mean of each sequence's last hidden states: EmbeddingModel::embed per sequence (embeddings.rs:396-447) */
int  fl_encoder_embed(fl_encoder *e, const uint32_t *ids, const size_t *offsets /* [n_seq + 1] */, size_t n_seq, float *out);
/* the unmasked ragged attention kernel alone on host buffers (unit tests): q/k/v [T_total][H*d] of `dtype` (FL_DTYPE_BF16: the MFMA
 * kernel, its bf16 output widened; FL_DTYPE_F32: the VALU kernel), d 32 or 64, out [T_total][H*d] fp32 */
int  fl_op_encoder_attention(const void *q, const void *k, const void *v, const size_t *offsets, size_t n_seq,
                             int64_t H, int64_t d, int32_t dtype, float *out);

/* The encoder's four row kernels alone on host buffers (unit tests).  fp32 matrices are row-major; `dtype` (FL_DTYPE_BF16 bits or
 * FL_DTYPE_F32) is the type of the tables of form 0 and of `out` in forms 0 to 2.
 *   form 0  launch_encoder_embed_ln: word [vocab][h], pos [P][h] and tt0 [h] (or NULL) in `dtype`, ids [T], offsets [n_seq + 1] with
 *           T = offsets[n_seq], ln_w / ln_b [h], eps; the row -> sequence table is built as the encoder's forward builds it
 *   form 1  launch_encoder_add_ln: x [T][h] (the residual stream), slabs [n_slab][T][h] (a projection's split-K slabs), bias [h] (or
 *           NULL), ln_w / ln_b [h], eps
 *   form 2  launch_encoder_bias_act: slabs [n_slab][T][h] (h: the row width N), bias [h] (or NULL), act (-1 none, or an fl_activation)
 *   form 3  launch_encoder_pool_l2: x [T][h], offsets [n_seq + 1] with T = offsets[n_seq]
 * x_res_out [T][h] fp32: the residual stream after forms 0 and 1.  out: forms 0 and 1 the normalised rows [T][h] and form 2 the
 * activation [T][h], as stored (`dtype`); form 3 the pooled rows [n_seq][h] fp32.  Every output is filled with the 0xff byte pattern
 * (NaN) before each launch -- but form 1's residual stream, which the kernel updates in place and which starts as x --; the `repeat`
 * launches (1..8) start from the same inputs: FL_ERR_HIP if one gives other bytes.
 * Decided before the device is probed, writing nothing: FL_ERR_BAD_ARGUMENT (null pointers, struct_size, form, dtype, act, repeat,
 * n_slab outside 1..8, sizes that are not positive, h not a multiple of 8 in forms 0 to 2, offsets that do not start at 0, decrease
 * or hold an empty sequence, an id >= vocab) and FL_ERR_SEQ_OVERFLOW (form 0: a sequence longer than P). */
typedef struct fl_encoder_rows_args {
    size_t struct_size;             /* sizeof(fl_encoder_rows_args) */
    int32_t form, dtype, n_slab, repeat;
    int32_t act, reserved;
    int64_t T, h, vocab, P;         /* T: forms 1 and 2 (forms 0 and 3 take it from offsets) */
    size_t n_seq;
    const void *word, *pos, *tt0;
    const uint32_t *ids;
    const size_t *offsets;
    const float *x, *slabs, *bias, *ln_w, *ln_b;
    float eps, reserved2;
    float *x_res_out;
    void *out;
} fl_encoder_rows_args;
int  fl_op_encoder_rows(const fl_encoder_rows_args *args);

/* Which slice of a full HF tensor does tp_rank own?  Pure host function (no GPU):
 * out = {row_begin, row_end, col_begin, col_end}.  Column-parallel q/k/v/gate/up/lm_head
 * (rows of the [out,in] matrix), row-parallel o_proj/down_proj (columns), everything else whole. */
int fl_tp_slice(const fl_config *cfg, const char *tensor_name, int32_t tp_rank, int32_t tp_size,
                int64_t out[4]);

/* ---- measurement hooks (bench.py / profiles) --------------------------------------------- */
typedef struct fl_kernel_stat {
    char    name[48];               /* kernel class, e.g. "gemv_bf16" */
    int64_t launches;
    double  total_ms;               /* sum of HIP-event durations (hipExtLaunchKernelGGL start/stop) */
    double  bytes;                  /* algorithmic HBM bytes over those launches */
    double  flops;                  /* algorithmic flops over those launches */
} fl_kernel_stat;
/* While profiling is on, forwards run eagerly and every kernel launch is bracketed by a HIP
 * event pair on the launch stream. */
int fl_profile_begin(fl_model *m);
int fl_profile_end(fl_model *m, fl_kernel_stat *stats, size_t cap, size_t *n_stats);

/* Times the small all-reduce of a decode step (n fp32 values, n <= hidden_size) on the links the group really has, one form at a
 * time: form 0 = ncclAllReduce (RCCL), 1 = the one-shot kernel over peer-mapped HBM (k_comm.hip), 2 = the exchange that rides in
 * the GEMV epilogues (comm_ll.h; timed through its stand-alone exerciser, one-shot epoch steps subtracted).  Collective: every
 * rank of the group calls it with the same arguments.  *us_per_call < 0: that form is not available in this group.
 * (the decode all-reduce after o_proj / down_proj; bench.py --gpus N reports the three side by side.) */
int fl_comm_probe(fl_model *m, int32_t form, int64_t n, int32_t iters, double *us_per_call);

/* Proves the one-shot collectives of a connected FL_TP_MULTI_PROCESS group on data whose sums are exact: one all-reduce of n
 * integer-valued floats (n <= FL_AR_INBOX_FLOATS; 16 384 and more take the many-workgroup form, fewer the one-workgroup form),
 * every wait bounded by 2 s.  Collective: every rank calls it with the same n.  *ok = 1: this rank holds the exact sums; 0: a wrong
 * sum or a wait that gave up (the error state is cleared: the group stays usable).  A model created with a unique_id has run this
 * itself (and fallen back by an all-ranks vote); a group wired by fl_comm_ipc_connect can ask for it here.
 * (the all-reduce after o_proj / down_proj.) */
int fl_comm_selftest(fl_model *m, int64_t n, int32_t *ok);

/* Process-wide switches (sweeps and tests; not needed in normal use).  Every switch is an integer row of ONE table
 * (fastllm_amd/csrc/common.h, enum TuneKey, documents each; DESIGN.md's appendix lists them): key "gemm_h4" is the row read from
 * the environment variable FL_GEMM_H4.  The environment is read ONCE, on first use; afterwards only this call changes a switch.
 *   value        >= 0, or -1 = "automatic" for the switches that have such a setting
 *   "reload_env" re-reads every FL_<NAME> from the environment (value ignored)
 *   "gemv_blocks" / "gemv_waves"  force the decode GEMV's grid / waves per workgroup (0 = automatic); "gemv_r" rows per wave pass
 *                (2|4) and "gemv_u" 512-element chunks per pipeline block (0 automatic, 2|4|7|8) are table rows like the rest
 *   "experimental"  FL_OK in the EXPERIMENTAL build (make EXPERIMENTAL=1), FL_ERR_UNSUPPORTED in the default one
 * FL_ERR_BAD_ARGUMENT: unknown key.  FL_ERR_UNSUPPORTED: the key belongs to a kernel that is compiled into the EXPERIMENTAL build
 * only (decode engine, fused attention + o_proj, attention prefetch workgroups, loader waves, "engine_grid"); the default build's
 * environment cannot reach those either. */
int fl_tune(const char *key, int value);

/* y[T,N] = x[T,K] . W[N,K]^T (+bias): the projection kernel family on host buffers, for unit
 * tests and micro-benchmarks.  dtype is the storage type of x and W (bf16 or f32); y is fp32.
 * epilogue: 0 none, 1 silu-gate (W rows are gate/up pairs in HF order: gate = rows [0,N/2),
 * up = rows [N/2,N); y is [T, N/2]).  iters > 0 with ms_out != NULL times `iters` launches. */
int fl_op_linear(const void *x, const void *w, const float *bias, int64_t T, int64_t N, int64_t K,
                 int32_t dtype, int32_t epilogue, float *y, int32_t iters, double *ms_out);

/* The FP8 row quantiser alone (unit tests): w host [N,K] of `dtype` (FL_DTYPE_F32 or FL_DTYPE_BF16), K a multiple of 4, through the
 * device kernel -> q_out [N,K] e4m3fn bytes and s_out [N] (the format of fl_weight_format above). */
int fl_op_quantize_rows(const void *w, int32_t dtype, int64_t N, int64_t K, uint8_t *q_out, float *s_out);

/* The FP8 decode weight stream alone (unit tests, micro-benchmarks): y[N] = s[n] * (q[n,:] . x) (+bias).  x host bf16 [K], q host
 * e4m3fn [N,K], s host fp32 [N], K a multiple of 16 (else FL_ERR_UNSUPPORTED); y fp32.  epilogue as fl_op_linear: 0 none, 1
 * silu-gate (q / s rows are gate/up in HF order, gate = rows [0,N/2); y is [N/2], the kernel's bf16 output widened).
 * iters > 0 with ms_out != NULL times `iters` launches over rotating copies of q, as fl_op_linear does. */
int fl_op_gemv_w8(const void *x, const uint8_t *q, const float *s, const float *bias, int64_t N, int64_t K, int32_t epilogue,
                  float *y, int32_t iters, double *ms_out);

/* ---- residual add -> RMSNorm -> projection in each of its fused forms, on host buffers (unit tests) ----------------------------- */

/* launch_rmsnorm_add alone: x_res [T][h] fp32 (updated in place: += the n_slab slabs of delta, summed in slab order), delta
 * [n_slab][T][h] fp32 (NULL with n_slab 0: x_res stays as it is), w [h] fp32.  xs_out [T][h] = x_res * w in `dtype`, widened to
 * fp32; inv_rms_out [T] = 1 / sqrt(mean(x_res^2) + eps).  h a multiple of 8; 0 <= n_slab <= 64. */
int fl_op_rmsnorm_add(float *x_res, const float *delta, int32_t n_slab, const float *w, float eps, int64_t T, int64_t h, int32_t dtype,
                      float *xs_out, float *inv_rms_out);

/* Kernel codes in the kernels_out arrays of the two calls below (fastllm_amd/csrc/kernels.h, enum LK_*). */
enum {
    FL_LK_NONE = 0, FL_LK_GEMV = 1, FL_LK_H4 = 2, FL_LK_W14 = 3, FL_LK_SKF = 4, FL_LK_DMA = 5, FL_LK_SKINNY = 6, FL_LK_8P = 7,
    FL_LK_8P_STREAMK = 8, FL_LK_256 = 9, FL_LK_128 = 10, FL_LK_4W_ROPE = 11, FL_LK_GENERIC = 12, FL_LK_F32_ROWS = 13, FL_LK_F32_MFMA = 14
};

/* The norm and ONE projection behind it, in the form the caller names -- never another one: a form that cannot run the request
 * returns FL_ERR_UNSUPPORTED.
 *   form 0  launch_rmsnorm_add, then launch_linear with row_scale = 1/rms (any T, bf16 / f32; every fl_tune switch as fl_op_linear)
 *   form 1  the single-sequence weight stream with its norm prologue (T = 1, bf16 / f32, K <= 6144)
 *   form 2  the same over FP8 weights: w = e4m3fn bytes [N][K], w_scale [N] as fl_op_quantize_rows gives them (T = 1, bf16, n_slab <= 1)
 *   form 3  the batched stream, T = B <= 8 rows, bf16; pro 0 runs its plain form on x instead of the norm
 * The normed vector is v = x_res + the delta slabs, added slab by slab in slab order in every form, or row
 * tokens[t] of embed when embed is given (x_res and delta NULL).  y [T][N] fp32, or [T][N/2] for epilogue 1 (w rows gate | up in HF
 * order, no bias), the kernel's output widened; x_out [T][K] (or NULL) = v.  repeat launches (1..8) run on the same buffers:
 * FL_ERR_HIP if one of them gives other bits.  kernels_out [4] (or NULL): form 0: {kernel, K slices, tail kernel, rest kernel} of the
 * plan (FL_LK_*; FL_LK_DMA for the FL_OP_LINEAR_DMA route); form 3: {0, K slices, 0, 0}. */
typedef struct fl_norm_linear_args {
    size_t struct_size;             /* sizeof(fl_norm_linear_args) */
    int32_t form, dtype, epilogue, pro;
    int64_t T, N, K;
    const float *x_res;             /* [T][K] fp32 */
    const void *x;                  /* form 3, pro 0: [T][K] bf16 */
    const float *delta;             /* [n_slab][T][K] fp32, or NULL */
    const float *norm_w;            /* [K] fp32 */
    const void *embed;              /* [vocab][K] in dtype, or NULL */
    const uint32_t *tokens;         /* [T], with embed */
    const void *w;                  /* [N][K] in dtype (form 2: e4m3fn bytes) */
    const float *w_scale;           /* form 2: [N] */
    const float *bias;              /* [N] or NULL */
    int64_t vocab;
    int32_t n_slab, repeat;
    float eps, reserved;
    float *y, *x_out;
    int32_t *kernels_out;
} fl_norm_linear_args;
int fl_op_norm_linear(const fl_norm_linear_args *args);

/* A projection with the residual epilogue (bf16): h = h_in + x . w^T (+bias), xn = bf16(h * w_next), partial sums of squares of h per
 * row -- on the kernel plan_resid picks under the current switches (FL_ERR_UNSUPPORTED when it picks none) -- then 1/rms by
 * launch_rms_finalize, or (lazy) left to the consumer as partial sums exactly as the forward pass leaves them.  The consumer
 * (optional): y2 = (xn . w2^T) * 1/rms through launch_linear, epi2 0 -> y2 [T][N2], epi2 1 (w2 rows gate | up in HF order) -> [T][N2/2].
 * h_out [T][N], xn_out [T][N] (widened), part_out [T][np] (np = 4 * ceil(N / 256)), inv_rms_out [T]: the finalized vector; lazy
 * with a consumer: whatever the consumer left there (NaN where it read the partial sums itself); lazy without one: finalized after
 * everything else was read.  repeat launches (1..8) run from the same h_in on the same buffers and workspaces: FL_ERR_HIP if one
 * gives other bits.  kernels_out [6] (or NULL) = {kernel, K slices, tail kernel, tail K slices, consumer kernel, consumer reads the
 * partial sums (0 / 1)} as FL_LK_* codes. */
typedef struct fl_linear_resid_args {
    size_t struct_size;             /* sizeof(fl_linear_resid_args) */
    int64_t T, N, K, N2;
    const void *x;                  /* [T][K] bf16 */
    const void *w;                  /* [N][K] bf16 */
    const float *bias;              /* [N] or NULL */
    const float *h_in;              /* [T][N] fp32 */
    const float *w_next;            /* [N] fp32 */
    const void *w2;                 /* [N2][N] bf16, or NULL: no consumer */
    float eps;
    int32_t lazy, epi2, repeat;
    float *h_out, *xn_out, *inv_rms_out, *part_out, *y2_out;
    int32_t *kernels_out;
} fl_linear_resid_args;
int fl_op_linear_resid(const fl_linear_resid_args *args);

/* The decode stream's residual epilogue and the prologue that consumes it (bf16, one row; k_gemv.hip EPI_RESID / PRO_XS).
 * mode 0, the producer alone: h_out = h_in + w . x, xs_out = bf16(h_out * w_next) (bits), cs_out [N/8] = the sum of squares of every 8
 *   consecutive h_out; delta_out [N]: the launch's `out` buffer, which it must leave as the NaN pattern it was filled with.
 * mode 1, the consumer alone on the caller's xs (bf16 bits) and cs: y = (w2 . xs) / sqrt(sum(cs) / N + eps) through epilogue epi2 --
 *   0: y_out [N2] fp32, and amax_out[0] = the row the launch's ArgMax candidates give (-1 where its grid leaves none); 1 (w2 rows
 *   gate | up in HF order): [N2/2] silu(gate) * up; 2 (N2 = (H + 2 Hkv) d): RoPE at `pos`, the row appended at slot `len` of a cache
 *   of seq_alloc positions (V transposed); y_out [N2] = q | the appended k row | the appended v row.
 * mode 2, the pair, next to today's two launches (plain epilogue, then the norm prologue) on the same inputs: the above, and h_ref,
 *   y_ref, amax_out[1] from those.
 * inv_out / inv_ref: the 1/m the prologue applied, read through a probe launch of the consumer's shape on the same sums (see
 * api_ops.hip).  FL_ERR_UNSUPPORTED where a launch does not take the form (a grid that does not cover N exactly, a forced grid,
 * fewer staging threads than N / 8).  repeat launches (1..8) run on the same buffers: FL_ERR_HIP if one gives other bytes. */
typedef struct fl_gemv_resid_args {
    size_t struct_size;             /* sizeof(fl_gemv_resid_args) */
    int32_t mode, epi2, repeat, reserved;
    int64_t N, K, N2;
    int64_t H, Hkv, d, max_pos, pos, len, seq_alloc;   /* epi2 2 */
    const void *x;                  /* [K] bf16 */
    const void *w;                  /* [N][K] bf16 */
    const float *h_in, *w_next;     /* [N] fp32 */
    const void *xs;                 /* mode 1: [N] bf16 */
    const float *cs;                /* mode 1: [N/8] */
    const void *w2;                 /* [N2][N] bf16 */
    const float *cos_tab, *sin_tab; /* epi2 2: [max_pos][d/2] */
    float eps, reserved2;
    float *h_out; void *xs_out; float *cs_out, *delta_out;
    float *y_out, *inv_out;
    float *h_ref, *y_ref, *inv_ref;
    int32_t *amax_out;              /* [2] or NULL */
} fl_gemv_resid_args;
int fl_op_gemv_resid(const fl_gemv_resid_args *args);

/* ---- QKV projection -> RoPE -> KV append in each of its forms, on host buffers (unit tests) -------------------------------------- */

/* The sequences of one call, shared by the two calls below.  Sequence s brings count[s] new rows (the rows of all sequences back to
 * back), rotated at positions pos[s] + t and appended at slots len[s] + t of its own cache: K [layers][Hkv][seq_alloc[s]][d] and V
 * the same, or transposed [layers][Hkv][d][seq_alloc[s]] where v_transposed[s] != 0, both in `dtype` (bf16 bits or fp32).  The caches
 * are passed in whole and come back whole, so a caller sees every element a kernel wrote outside the appended slots.  Only layer
 * `layer` of `layers` is written.  Both calls return FL_ERR_BAD_ARGUMENT before the device is touched for len[s] + count[s] >
 * seq_alloc[s], pos[s] + count[s] > max_pos, an odd d, H not a multiple of Hkv and layer >= layers, and FL_ERR_UNSUPPORTED for what
 * the named form cannot take. */
typedef struct fl_rope_seqs {
    int32_t n_seq, layers, layer, reserved;
    const int32_t *count, *pos, *len, *seq_alloc, *v_transposed;   /* [n_seq] each */
    void *const *k_cache, *const *v_cache;                         /* [n_seq] host caches, updated in place */
} fl_rope_seqs;

/* The stand-alone RoPE + KV-append kernels.  qkv fp32 [n_slab][rows][(H + 2 Hkv) * d] (the K slabs of a projection, summed in slab
 * order; then the optional bias [(H + 2 Hkv) * d]), cos_tab / sin_tab fp32 [max_pos][d / 2]; q_out [rows][H * d] in `dtype`.
 *   form 0  launch_rope_kv: one sequence (the vector kernel where its own rule takes it, else the scalar one)
 *   form 1  launch_rope_kv_batch: count[s] = 1 for every s, one layout for all sequences (fp32: row-major V only)
 *   form 2  launch_rope_kv_packed: any counts, the layout per sequence
 * repeat launches (1..8) start from the same caches: FL_ERR_HIP if one gives other bytes.  kernels_out [4] (or NULL) = {0 scalar /
 * 1 vector / 2 batch / 3 packed, dtype, V transposed (forms 0 and 1), workgroups of the vector kernel's q / k part (else 0)}. */
typedef struct fl_rope_kv_args {
    size_t struct_size;             /* sizeof(fl_rope_kv_args) */
    int32_t form, dtype, n_slab, repeat;
    int64_t H, Hkv, d, max_pos;
    const float *qkv, *bias, *cos_tab, *sin_tab;
    fl_rope_seqs seqs;
    void *q_out;
    int32_t *kernels_out;
} fl_rope_kv_args;
int fl_op_rope_kv(const fl_rope_kv_args *args);

/* Residual add -> RMSNorm -> QKV projection with RoPE and the KV append behind it; the inputs as fl_norm_linear_args (N = (H + 2 Hkv) * d).
 *   form 0  a prompt of T rows as the forward pass runs it: launch_rmsnorm_add, plan_qkv_rope, then the planned kernel with the
 *           epilogue -- or, where the plan keeps fp32 slabs, the plain projection and launch_rope_kv over the slabs (one sequence)
 *   form 1  the single-sequence weight stream, norm prologue and RoPE epilogue (T = 1, K <= 6144)
 *   form 2  the same over FP8 weights (T = 1, bf16, n_slab <= 1)
 *   form 3  the batched stream: T = n_seq <= 8 rows, one sequence each, bf16, transposed V
 * q_out [T][H * d] in `dtype`; x_out [T][K] (or NULL) = the normed vector's input v; repeat as above.  kernels_out [4] (or NULL):
 * form 0: {kernel, K slices, tail kernel, 1 if the epilogue ran in the projection else 0} (FL_LK_*); the weight streams (forms 1 to 3): {FL_LK_GEMV, 1, 0, 1}. */
typedef struct fl_qkv_rope_args {
    size_t struct_size;             /* sizeof(fl_qkv_rope_args) */
    int32_t form, dtype, n_slab, repeat;
    int64_t T, K, H, Hkv, d, max_pos, vocab;
    const float *x_res;             /* [T][K] fp32 */
    const float *delta;             /* [n_slab][T][K] fp32, or NULL */
    const float *norm_w;            /* [K] fp32 */
    const void *embed;              /* [vocab][K] in dtype, or NULL */
    const uint32_t *tokens;         /* [T], with embed */
    const void *w;                  /* [N][K] in dtype (form 2: e4m3fn bytes) */
    const float *w_scale;           /* form 2: [N] */
    const float *bias;              /* [N] or NULL */
    const float *cos_tab, *sin_tab;
    float eps, reserved;
    fl_rope_seqs seqs;
    void *q_out;
    float *x_out;
    int32_t *kernels_out;
} fl_qkv_rope_args;
int fl_op_qkv_rope(const fl_qkv_rope_args *args);

/* ---- decode attention replicated inside the o_proj launch (short caches), on host buffers (unit tests) ---------------------------- */

/* launch_attn_oproj_rep alone, called as the decode step calls it (scale = 1 / sqrt(d), no tensor-parallel epilogue): out = w_o .
 * attention(q, K, V), the attention output rounded to bf16 in between.  All operands are bf16 bits: q [H * d]; k / v [k_rows][Hkv * d]
 * row-major, of which the kernel sees the first S = s_past + 1 rows (the rows behind are stale cache contents); w_o [N][H * d].  The
 * call builds the cache in the model's layout, K [Hkv][sa][d] and V transposed [Hkv][d][sa] with sa = capacity rounded up to 32;
 * rows k_rows .. sa hold pad_value (finite).  S <= k_rows <= capacity.  out fp32 [repeat][N]: each of the `repeat` launches (1..16)
 * writes a row of its own, which is filled with the 0xff byte pattern (NaN) first.
 * info_out [6] (or NULL) = {1 if the decode step would take this launch for a cache of sa rows, 1 if it would with FL_ATTN_REP=2
 * (any size), rows per wave, head slots per wave slab (GMAX), workgroups, key slices per kv head}.  query_only = 1: fill info_out and
 * return; no pointer but info_out is read, s_past and k_rows are ignored and the device is not touched.
 * FL_ERR_BAD_ARGUMENT (null pointers, struct_size, sizes out of range, H not a multiple of Hkv, a pad_value that is not finite,
 * repeat) and FL_ERR_UNSUPPORTED (head_dim other than 64 / 128, more than 8 query heads per kv head, 8 not a multiple of Hkv, H * d
 * above 2048; without query_only also a capacity of more than 32 key tiles per slice) come back before the device is probed and write
 * nothing. */
typedef struct fl_attn_oproj_rep_args {
    size_t struct_size;             /* sizeof(fl_attn_oproj_rep_args) */
    int64_t H, Hkv, d, N, s_past, k_rows, capacity;
    const void *q, *k, *v, *w_o;
    float pad_value;
    int32_t repeat, query_only, reserved;
    float *out;
    int32_t *info_out;
} fl_attn_oproj_rep_args;
int fl_op_attn_oproj_rep(const fl_attn_oproj_rep_args *args);

/* The token-selection kernel alone, for unit tests: `n_draws` successive selections from one host logits
 * vector (consuming successive words of the seeded stream; ArgMax when temperature < 1e-7). */
int fl_op_sample(const float *logits, int64_t V, const fl_sampling *sampling, int64_t n_draws, uint32_t *tokens_out);

/* ... with an fl_sampler; kept_out (optional, [n_draws]): how many tokens each draw kept (V when no filter is on) */
int fl_op_sample_ex(const float *logits, int64_t V, const fl_sampler *sampler, int64_t n_draws, uint32_t *tokens_out, int64_t *kept_out);

/* The selection kernel of fl_forward_verify alone, on host logits (unit tests): argmax_out[t] = ArgMax of row t (ties -> LAST maximal
 * index), *n_accepted_out = the largest j <= T - 1 with draft[i] == argmax_out[i] for all i < j.  1 <= T <= FL_VERIFY_MAX_DRAFT + 1;
 * draft may be NULL when T == 1. */
int fl_op_verify_select(const float *logits /* [T][V] */, int64_t T, int64_t V, const uint32_t *draft /* [T-1] */,
                        uint32_t *argmax_out /* [T] */, int64_t *n_accepted_out);

/* The selection kernel of a sampled fl_forward_verify_ex alone, on host logits (unit tests, tools): tokens_out[t] = the draw of row t
 * with word sampler->draws_done + t -- what fl_op_sample_ex gives for that row with that draws_done -- and *n_accepted_out as above.
 * kept_out (or NULL, [T]): how many tokens each row's filter kept (V when none is on).  temperature < 1e-7: FL_ERR_BAD_ARGUMENT
 * (that is fl_op_verify_select).  Launched twice on the same buffers: FL_ERR_HIP if the two results differ. */
int fl_op_verify_sample(const float *logits /* [T][V] */, int64_t T, int64_t V, const uint32_t *draft /* [T-1] */, const fl_sampler *sampler,
                        uint32_t *tokens_out /* [T] */, int64_t *n_accepted_out, int64_t *kept_out /* [T] or NULL */);
/* ... and timed (tools/verify_sample_cost.py): ms_out[0] = ms per launch of that kernel on the T rows, ms_out[1] = ms per T one-row
 * selection launches (select_advance) of the same rows, each the mean of iters[form] back-to-back repetitions between two events
 * (0: that form is not run, ms_out[form] = 0). */
int fl_op_verify_sample_time(const float *logits /* [T][V] */, int64_t T, int64_t V, const fl_sampler *sampler,
                             const int32_t *iters /* [2] */, double *ms_out /* [2] */);

/* The selection kernel of fl_batch_verify alone, on host logits (unit tests, tools): a pack of n_seq members, member s = rows
 * offsets[s] .. offsets[s+1] with ids [token, draft ..]; samplers[s] (NULL: ArgMax for all; temperature < 1e-7: ArgMax) selects its
 * rows -- row i of a sampled member is what fl_op_sample_ex gives for that row with draws_done + i.  The rows are cut into launches
 * of block_rows rows (0: one launch), so a member may straddle launches.  tokens_out[r]: row r's id; n_acc_out[s]: the largest
 * j <= count_s - 1 with ids[offsets[s] + 1 + k] == tokens_out[offsets[s] + k] for all k < j; kept_out (or NULL): what each row's
 * filter kept (V without one).  1 <= T <= 1024, 1 <= n_seq <= 64, members of 1 .. 16 rows, offsets[n_seq] == T, ids < V
 * (FL_ERR_BAD_ARGUMENT otherwise, before the device is probed).  Everything runs twice on the same buffers: FL_ERR_HIP if the two
 * results differ.  iters > 0 with ms_out: the launches of one pass timed between two events, ms per pass. */
int fl_op_verify_packed(const float *logits /* [T][V] */, int64_t T, int64_t V, size_t n_seq, const size_t *offsets /* [n_seq+1] */,
                        const uint32_t *ids /* [T] */, const fl_sampler *samplers /* [n_seq] or NULL */, int64_t block_rows /* 0: one launch */,
                        uint32_t *tokens_out /* [T] */, int64_t *n_acc_out /* [n_seq] */, int64_t *kept_out /* [T] or NULL */,
                        int32_t iters, double *ms_out);

/* The log-prob kernel of the fl_*_lp calls alone, on host logits (unit tests, micro-benchmarks): row t's chosen token is chosen[t].
 * 1 <= T <= 64, 0 <= top_n <= min(FL_LOGPROBS_MAX_TOP, V), V <= 1 << 24, chosen[t] < V (FL_ERR_BAD_ARGUMENT otherwise, before the
 * device is probed); top_ids / top_logprobs may be NULL when top_n == 0.  Launched twice: FL_ERR_HIP if the two results differ. */
int fl_op_logprobs(const float *logits /* [T][V] */, int64_t T, int64_t V, const uint32_t *chosen /* [T] */, int32_t top_n,
                   float *token_logprob /* [T] */, uint32_t *top_ids /* [T][top_n] or NULL */, float *top_logprobs /* [T][top_n] or NULL */);

/* The scoring kernel of fl_forward_score / fl_batch_score alone, on host logits (unit tests, micro-benchmarks): row t's target is
 * targets[t] (FL_SCORE_NO_TARGET: none).  1 <= T <= 1024, 0 <= top_n <= min(FL_LOGPROBS_MAX_TOP, V), V <= 1 << 24, targets[t] < V or
 * the sentinel (FL_ERR_BAD_ARGUMENT otherwise, before the device is probed); target_rank may be NULL, top_ids / top_logprobs when
 * top_n == 0.  Launched twice: FL_ERR_HIP if the two results differ. */
int fl_op_score(const float *logits /* [T][V] */, int64_t T, int64_t V, const uint32_t *targets /* [T] */, int32_t top_n,
                float *target_logprob /* [T] */, uint32_t *target_rank /* [T] or NULL */, uint32_t *top_ids /* [T][top_n] or NULL */,
                float *top_logprobs /* [T][top_n] or NULL */);
/* ... and timed (tools/score_cost.py): *ms_out = ms per launch on the T rows, the mean of `iters` back-to-back launches between two events */
int fl_op_score_time(const float *logits /* [T][V] */, int64_t T, int64_t V, const uint32_t *targets /* [T] */, int32_t top_n, int32_t iters,
                     double *ms_out);

/* The logit-rules kernel alone, on host arrays (unit tests): the batch form on B rows of V logits.  Row b has its own table
 * (words / biases [B][V]; words in/out: the counted word comes back) and scalars scalars[b] = {repetition, frequency, presence
 * penalty}; tokens[b] is the row's input token, counted when count_input != 0 (an id >= V: none).  has_rules (optional, [B]): 0 makes
 * row b's table entry null, and the row is copied through.  1 <= B <= 64, 1 <= V <= 1 << 24, FL_ERR_BAD_ARGUMENT otherwise (before
 * the device is probed). */
int fl_op_logit_rules(const float *logits /* [B][V] */, int64_t B, int64_t V, uint32_t *words /* [B][V] */, const float *biases /* [B][V] */,
                      const float *scalars /* [B][3] */, const uint32_t *tokens /* [B] */, int32_t count_input,
                      const uint8_t *has_rules /* [B] or NULL */, float *out /* [B][V] */);

/* The guided-decoding kernel alone, on host arrays (unit tests): the batch form on B rows of V logits and one automaton (the CSR
 * arrays of fl_guide_desc, validated as fl_guide_create validates them against this V).  Row b enters in states[b] (< n_states), first
 * moves along the edge of tokens[b] as a decode step moves along its input token (no such edge, or an id >= V: it stays), and is masked
 * in the state it reached, which comes back in next_states[b].  has_guide (optional, [B]): 0 makes row b's control block null, and the
 * row is copied through (next_states[b] = states[b]).  1 <= B <= 64, 1 <= V <= 1 << 24, FL_ERR_BAD_ARGUMENT otherwise (before the
 * device is probed).  Launched twice: FL_ERR_HIP if the two results differ. */
int fl_op_guide_mask(const float *logits /* [B][V] */, int64_t B, int64_t V, const fl_guide_desc *desc, const uint32_t *states /* [B] */,
                     const uint32_t *tokens /* [B] */, const uint8_t *has_guide /* [B] or NULL */, float *out /* [B][V] */,
                     uint32_t *next_states /* [B] */);

/* verify_adjust_kernel alone, on host arrays (unit tests, tools/verify_adjust_cost.py): the rows of one verify step, logits [T][V],
 * 1 <= T <= 16, row i's input id ids[i] (>= V: counts nothing).  Rules (words != NULL; then biases [V] and scalars = {repetition,
 * frequency, presence penalty} too): row i is adjusted with each table word counted once per r <= i with ids[r] == its id; words is
 * in/out and comes back AS THE LAUNCHES LEFT IT, i.e. unchanged.  Guide (desc != NULL, validated as fl_guide_create validates it
 * against this V; states [T] < n_states): row i is masked in states[i].  At least one of the two; 1 <= V <= 1 << 24;
 * FL_ERR_BAD_ARGUMENT otherwise (before the device is probed).  Launched twice: FL_ERR_HIP if the two results differ. */
int fl_op_verify_adjust(const float *logits /* [T][V] */, int64_t T, int64_t V, const uint32_t *ids /* [T] */, uint32_t *words /* [V] or NULL */,
                        const float *biases /* [V] */, const float *scalars /* [3] */, const fl_guide_desc *desc /* or NULL */,
                        const uint32_t *states /* [T] */, float *out /* [T][V] */);
/* ... and timed (tools/verify_adjust_cost.py): *ms_out = ms per launch on the T rows, the mean of `iters` back-to-back launches between two
 * events; nothing comes back and words is not written. */
int fl_op_verify_adjust_time(const float *logits /* [T][V] */, int64_t T, int64_t V, const uint32_t *ids /* [T] */, const uint32_t *words,
                             const float *biases, const float *scalars, const fl_guide_desc *desc, const uint32_t *states, int32_t iters,
                             double *ms_out);
/* rules_count_kernel alone: ids[0 .. n), 0 <= n <= 16, counted into words [V] in order (saturating; an id >= V counts nothing). */
int fl_op_rules_count(uint32_t *words /* [V] in/out */, int64_t V, const uint32_t *ids /* [n] */, int64_t n);

/* The copy kernel of fl_cache_copy_prefix alone on host buffers (unit tests, micro-benchmarks): `rows` rows of `width_bytes` bytes go
 * from src (rows * src_pitch bytes) to dst (rows * dst_pitch bytes).  dst is in/out: it is uploaded, the kernel runs, and it is read
 * back, so the bytes the kernel must not touch -- everything outside [0, width_bytes) of a row -- can be checked.  rows >= 1;
 * width_bytes >= 2 and a multiple of 2; both pitches multiples of 16 and at least width_bytes; anything else FL_ERR_BAD_ARGUMENT
 * (before the device is touched).  iters > 0 with ms_out != NULL times `iters` launches over rotating buffer pairs, as fl_op_linear. */
int fl_op_kv_copy(const void *src, void *dst, int64_t rows, int64_t width_bytes, int64_t src_pitch, int64_t dst_pitch,
                  int32_t iters, double *ms_out);

/* The bf16 MFMA attention kernels alone, for unit tests against an fp64 reference (they are otherwise only seen through
 * whole-model logits).  One sequence: q [T][H*d] (RoPE already applied), k / v [s_past + T][Hkv*d], all bf16 row-major; the
 * first s_past positions are the cache, the last T the new tokens.  Mask as the forward pass applies it:
 * T == 1: no mask; T > 1: cached keys visible, new key j visible to query t iff j <= t and j + window >= t (window < 0: no
 * window).  kernel: 0 = what the model would launch, 1 = decode kernel (T must be 1), 2 = 16-row prefill kernel, 3 =
 * 32-row prefill kernel.  nsplit: key splits of the decode kernel (0 = as fl_cache_create picks; 1 = one wide workgroup
 * per kv head).  out [T][H*d] fp32 (the kernels' bf16 output widened). */
int fl_op_attention(const void *q, const void *k, const void *v, int64_t T, int64_t s_past, int64_t H, int64_t Hkv,
                    int64_t d, int64_t window, int32_t kernel, int32_t nsplit, float *out);

/* The attention launches of the model on caches built here from host buffers, for unit tests: the plain-layout (VALU) kernels of
 * every fp32 model and of the bf16 head shapes the MFMA kernels refuse (layout 0; dtype FL_DTYPE_BF16 or FL_DTYPE_F32), or the bf16
 * MFMA kernels of fl_op_attention (layout 1: V transposed, FL_DTYPE_BF16, at most 8 query heads per kv head).  One sequence: q
 * [T][H*d], k / v [k_rows][Hkv*d] of `dtype`, row-major.  The cache gets `capacity` positions (rounded up to 32 as fl_cache_create
 * does): rows [0, s_past) are the cached prefix, [s_past, s_past + T) the call's tokens, rows [s_past + T, k_rows) are stale
 * contents behind the cached length (what fl_cache_truncate or a speculative rollback leaves), and every position from k_rows on
 * holds pad_value (finite).  call0 <= s_past: the cached length when the API call began -- below s_past it is the mask of a later
 * chunk of a prefill the library cut up: keys below call0 are visible, key j >= call0 is visible to the query at position p iff
 * j <= p and j + window >= p (window < 0: none; T == 1 through the decode kernel: no mask).  kernel: 0 = what the model would
 * launch, 1 = decode (T must be 1), 2 = prefill (layout 1: the 16-row kernel), 3 = the 32-row prefill kernel (layout 1 only).
 * nsplit: key splits of the decode kernel, 1..64, 0 = what fl_cache_create picks for `capacity`; the workgroup width of the plain
 * decode kernel is the attn_nw switch (fl_tune).  `repeat` (1..16) launches run on ONE split scratch and one set of ticket words;
 * out [repeat][T][H*d] fp32 holds every launch's output (pre-filled with the 0xff pattern, bf16 widened).  Argument errors are
 * FL_ERR_BAD_ARGUMENT, head shapes no kernel takes (d other than 64 / 128, layout 1 with fp32 or more than 8 heads per kv head)
 * FL_ERR_UNSUPPORTED, both before the device is touched. */
int fl_op_attention_plain(const void *q, const void *k, const void *v, int32_t dtype, int32_t layout, int32_t kernel, int64_t T,
                          int64_t s_past, int64_t call0, int64_t k_rows, int64_t capacity, int64_t H, int64_t Hkv, int64_t d,
                          int64_t window, int32_t nsplit, float pad_value, int32_t repeat, float *out);

/* The batched decode attention launches alone (unit tests): layout 0 = the plain-layout kernel (bf16 or fp32), layout 1 = the MFMA
 * kernel (bf16, V transposed).  B sequences, each with a cache of its own as fl_batch_create finds them: k[b] / v[b] are host rows
 * [n_layers][k_rows[b]][Hkv*d] of `dtype`; sequence b sees keys [0, lens[b]) of layer `layer` (the last of them is the step's own
 * token), rows [lens[b], k_rows[b]) are stale contents, positions from k_rows[b] to seq_alloc[b] (a multiple of 32) hold pad_value
 * in every layer.  nsplit[b]: the sequence's split count, 1..64, 0 = what fl_cache_create picks for a cache of seq_alloc[b]
 * positions; its split scratch and ticket words are sized for it.  The MFMA launch caps the splits by the attn_batch_wgs switch
 * (fl_tune) as in the model.  q [B][H*d]; out [repeat][B][H*d] fp32, `repeat` launches on the same scratch as above.  Errors as
 * fl_op_attention_plain. */
int fl_op_attention_batch(const void *q, const void *const *k, const void *const *v, int32_t dtype, int32_t layout, int64_t B,
                          const int64_t *lens, const int64_t *k_rows, const int64_t *seq_alloc, const int32_t *nsplit,
                          int64_t n_layers, int64_t layer, int64_t H, int64_t Hkv, int64_t d, float pad_value, int32_t repeat,
                          float *out);

/* The packed prefill attention launch alone (unit tests), in the style of fl_op_attention_batch: bf16, MFMA layout (V transposed).
 * q [T_total][H*d] packed by offsets; sequence s has a cache of its own, built here from host rows k[s] / v[s]
 * [n_layers][k_rows[s]][Hkv*d]: rows [0, s_past[s]) are its cached prefix, the next (offsets[s+1]-offsets[s]) its new tokens, rows
 * up to k_rows[s] stale contents, positions from k_rows[s] to seq_alloc[s] (a multiple of 32) hold pad_value in every layer.
 * window < 0: none.  out [T_total][H*d] fp32 (bf16 widened, pre-filled with the 0xff pattern).  1 <= n_seq <= 1023.  Errors as
 * fl_op_attention_batch. */
int fl_op_attention_packed(const void *q, const void *const *k, const void *const *v, int64_t n_seq, const int64_t *offsets,
                           const int64_t *s_past, const int64_t *k_rows, const int64_t *seq_alloc, int64_t n_layers, int64_t layer,
                           int64_t H, int64_t Hkv, int64_t d, int64_t window, float pad_value, float *out);
/* ... with the mask chosen: mask 0 (FL_MASK_CAUSAL) launches exactly what fl_op_attention_packed launches; 1 (FL_MASK_FULL): every
 * new token of a sequence sees all of its keys [0, s_past + new tokens), `window` is ignored. */
int fl_op_attention_packed_ex(const void *q, const void *const *k, const void *const *v, int64_t n_seq, const int64_t *offsets,
                              const int64_t *s_past, const int64_t *k_rows, const int64_t *seq_alloc, int64_t n_layers, int64_t layer,
                              int64_t H, int64_t Hkv, int64_t d, int64_t window, float pad_value, int32_t mask, float *out);

/* The pooling launch of fl_batch_embed alone, on host buffers (unit tests, micro-benchmarks): x [T][h] the fp32 residual rows,
 * inv_rms [T], w [h] the final norm's weight, offsets [n_seq + 1] (from 0 to T, increasing); opts as fl_batch_embed's (mask is not
 * looked at).  out: [n_seq][dims], or [T][dims] with FL_POOL_NONE; pre-filled with the 0xff pattern on the device.  h 1 .. 65536,
 * T 1 .. 2^20.  The launch runs twice and the two results must agree bit for bit (FL_ERR_HIP otherwise).
 * fl_op_pool_rows_time: the same launch(es) `iters` times between two events, *ms_out = ms per pool; nothing is downloaded. */
int fl_op_pool_rows(const float *x, const float *inv_rms, const float *w, const size_t *offsets, size_t n_seq, int64_t h,
                    const fl_embed *opts, float *out);
int fl_op_pool_rows_time(const float *x, const float *inv_rms, const float *w, const size_t *offsets, size_t n_seq, int64_t h,
                         const fl_embed *opts, int32_t iters, double *ms_out);

/* The weight conversion launch of the model build alone, on host buffers (unit tests): the slice [r0, r0 + rows) x [c0, c0 + cols) of
 * src [R][C] (src_dtype: f32 / bf16 / f16) goes, converted to dst_dtype (bf16 / f32), into dst [dst_rows][dst_ld].
 *   row_mode 0  source row r lands in row dst_row0 + r
 *            1  ... in the gate row of the 16 x 16 gate/up interleave, (r / 16) * 32 + r % 16;  2: in the up row, 16 further
 *               (dst_row0 must be 0: the interleave has no offset)
 *   head_pad 0  none;  1: the ROWS are heads of dm, laid out as heads of d: element j of a head goes to j (j < dm / 2) or to
 *               d / 2 + j - dm / 2 (row_mode must be 0);  2: the COLUMNS are
 *   via_bf16    fp32 destinations only: the value is rounded to bf16 first (how a bf16 model holds its norm weights and biases)
 * dst is output only: the device buffer is filled with 0xff bytes before the launch and returned whole, so the elements the launch
 * left alone show.  FL_ERR_BAD_ARGUMENT, before the device is touched, for a slice that leaves the source, for ANY element whose
 * destination is outside dst, for head_pad without 2 <= dm <= d (both even), and for more than 2^26 elements on either side. */
typedef struct fl_convert_slice_args {
    size_t struct_size;          /* sizeof(fl_convert_slice_args) */
    int32_t src_dtype, dst_dtype, row_mode, head_pad, via_bf16, reserved;
    int64_t R, C;                /* the source matrix */
    int64_t r0, c0, rows, cols;  /* the slice */
    int64_t dst_rows, dst_ld, dst_row0;
    int64_t dm, d;               /* head_pad 1 / 2 only */
    const void *src;
    void *dst;
} fl_convert_slice_args;
int fl_op_convert_slice(const fl_convert_slice_args *args);

/* One device tensor of a built model, copied to the host as it lies in HBM (unit tests of the model build: weights.hip's layout).
 * shard: index among the model's LOCAL shards (0 without tensor parallelism; the rank under FL_TP_SINGLE_PROCESS / FL_TP_EMULATED).
 * layer is looked at for the per-layer selectors only.  *rows_out, *cols_out, *elem_out (an fl_dtype, or FL_ELEM_E4M3: one byte per
 * element) are always written; out == NULL returns only those, otherwise out takes rows x cols elements.  The FL_MT_*_Q (e4m3 bytes)
 * and FL_MT_*_S (fp32 row scales, [rows][1]) selectors exist for FL_WEIGHTS_E4M3_ROW models, FL_MT_BQKV for models with q/k/v bias;
 * a selector the model does not have, a bad shard or a bad layer: FL_ERR_BAD_ARGUMENT.  The call takes the model's lock, waits for
 * the shard's stream and copies; it launches nothing. */
enum { FL_ELEM_E4M3 = 3 };
typedef enum fl_model_tensor_sel {
    FL_MT_EMBED = 0, FL_MT_NORM = 1, FL_MT_LM_HEAD = 2, FL_MT_COS_TAB = 3, FL_MT_SIN_TAB = 4,
    FL_MT_WQKV = 5, FL_MT_BQKV = 6, FL_MT_WO = 7, FL_MT_WGU = 8, FL_MT_WD = 9, FL_MT_LN1 = 10, FL_MT_LN2 = 11,
    FL_MT_WQKV_Q = 12, FL_MT_WQKV_S = 13, FL_MT_WO_Q = 14, FL_MT_WO_S = 15, FL_MT_WGU_Q = 16, FL_MT_WGU_S = 17,
    FL_MT_WD_Q = 18, FL_MT_WD_S = 19, FL_MT_LM_HEAD_Q = 20, FL_MT_LM_HEAD_S = 21
} fl_model_tensor_sel;
int fl_op_model_tensor(fl_model *m, int32_t shard, int32_t selector, int64_t layer, void *out, int64_t *rows_out, int64_t *cols_out,
                       int32_t *elem_out);

#ifdef __cplusplus
}
#endif
#endif
