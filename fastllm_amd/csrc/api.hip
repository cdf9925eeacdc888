// api.hip -- the extern "C" surface declared in include/fastllm_mi355x.h.
//
// Every entry point is an exception barrier: the host of this library is Rust (or ctypes), and a C++
// exception that crosses the C ABI is undefined behaviour there.  The reference surfaces failures as
// anyhow::Error (mod.rs:402-405,446-451); here std::bad_alloc becomes FL_ERR_OOM and anything else
// FL_ERR_HIP, both with fl_last_error() set (api_internal.h: guarded).  The fl_op_* entry points of the tests and tools/ are in
// api_ops.hip.
#include <vector>

#include "api_internal.h"
#include "encoder.h"
#include "lookup.h"

using namespace fl;

extern "C" {

int fl_abi_version(void) { return FL_ABI_VERSION; }
const char *fl_last_error(void) { return last_error(); }

int fl_device_count(int *count) {
    return guarded([&]() -> int {
        if (!count) FL_FAIL(FL_ERR_BAD_ARGUMENT, "null count");
        int n = 0;
        if (hipGetDeviceCount(&n) != hipSuccess) { (void)hipGetLastError(); n = 0; }
        *count = n;
        return FL_OK;
    });
}

int fl_comm_unique_id(void *out) {
    return guarded([&]() -> int {
        if (!out) FL_FAIL(FL_ERR_BAD_ARGUMENT, "null out");
        static_assert(sizeof(ncclUniqueId) <= FL_UNIQUE_ID_BYTES, "unique id size");
        ncclUniqueId id;
        ncclResult_t r = ncclGetUniqueId(&id);
        if (r != ncclSuccess) FL_FAIL(FL_ERR_RCCL, "ncclGetUniqueId: %s", ncclGetErrorString(r));
        memset(out, 0, FL_UNIQUE_ID_BYTES);
        memcpy(out, &id, sizeof id);
        return FL_OK;
    });
}

int fl_comm_ipc_export(fl_model *m, void *handle_out) {
    return guarded([&]() -> int {
        return comm_ipc_export(M(m), handle_out);
    });
}
int fl_comm_ipc_connect(fl_model *m, const void *handles) {
    return guarded([&]() -> int {
        return comm_ipc_connect(M(m), handles);
    });
}

int fl_model_create(const fl_config *cfg, const fl_tensor *tensors, size_t n_tensors, int32_t compute_dtype,
                    const fl_parallel *par, fl_model **out) {
    return guarded([&]() -> int {
        if (!out) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_model_create: null out");
        *out = nullptr;
        Model *m = nullptr;
        int rc = model_create(cfg, tensors, n_tensors, compute_dtype, par, nullptr, &m);
        if (rc == FL_OK) *out = reinterpret_cast<fl_model *>(m);
        return rc;
    });
}

int fl_model_create_opts(const fl_config *cfg, const fl_tensor *tensors, size_t n_tensors, int32_t compute_dtype,
                         const fl_parallel *par, const fl_model_options *opts, fl_model **out) {
    return guarded([&]() -> int {
        if (!out) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_model_create_opts: null out");
        *out = nullptr;
        Model *m = nullptr;
        int rc = model_create(cfg, tensors, n_tensors, compute_dtype, par, opts, &m);
        if (rc == FL_OK) *out = reinterpret_cast<fl_model *>(m);
        return rc;
    });
}

void fl_model_retain(fl_model *m) {
    guarded_void([&]() {
        if (m) M(m)->refs.fetch_add(1);
    });
}
void fl_model_release(fl_model *m) {
    guarded_void([&]() {
        if (m && M(m)->refs.fetch_sub(1) == 1) delete M(m);
    });
}

int fl_model_get_info(const fl_model *m, fl_model_info *out) {
    return guarded([&]() -> int {
        if (!m || !out) FL_FAIL(FL_ERR_BAD_ARGUMENT, "null argument");
        const Model *mm = M(m);
        const Dims &D = mm->D;
        memset(out, 0, sizeof *out);
        out->cfg = mm->cfg_resolved;
        out->head_dim = D.dm;                                    // the model's (the kernels may run it padded to 64 / 128)
        out->compute_dtype = mm->dtype;
        out->tp_size = mm->tp;
        const int64_t es = (int64_t)mm->esize();
        // weights read once per decoded token (one embedding row, norms, biases
        // included; the rest of the embedding table excluded)
        int64_t per_layer = 2 * D.h * D.h + 2 * D.Hkv * D.dm * D.h + 3 * D.h * D.inter;
        int64_t small = 2 * D.h + (D.qkv_bias ? D.h + 2 * D.Hkv * D.dm : 0);
        out->weight_bytes_per_token = es * (D.L * (per_layer + small) + D.h + D.V * D.h);
        out->decode_weights = mm->decode_weights;
        if (mm->decode_weights == FL_WEIGHTS_E4M3_ROW) {
            // what the FP8 step streams: 1 byte per projection weight and one fp32 scale per projection row; the embedding row,
            // norms and biases as before
            const int64_t rows = D.h + 2 * D.Hkv * D.dm + D.h + 2 * D.inter + D.h;      // q | k, v | o | gate, up | down
            out->weight_bytes_per_token = D.L * (per_layer + 4 * rows + es * small) + es * D.h + D.V * D.h + 4 * D.V;
        }
        out->kv_bytes_per_position = es * D.L * D.Hkv * D.dm * 2;
        out->hbm_bytes_allocated = mm->hbm_bytes;
        // + the GEMM workspaces of each shard's streams (first long prompt).  The workspace tables are keyed by (current device,
        // stream): the calling thread's device is put back afterwards, and forward() is kept out meanwhile (it sets devices too).
        std::lock_guard<std::mutex> lock(const_cast<Model *>(mm)->mu);
        int dev0 = -1;
        (void)hipGetDevice(&dev0);
        struct Restore { int d; ~Restore() { if (d >= 0) (void)hipSetDevice(d); } } restore{dev0};
        for (auto &sh : mm->shards) {
            if (hipSetDevice(sh.device) != hipSuccess) continue;
            out->hbm_bytes_allocated += gemm_8p_workspace_bytes(sh.stream) + gemm_8p_workspace_bytes(sh.comm_stream) + gemm_h4_workspace_bytes(sh.stream) +
                                        gemm_h4_workspace_bytes(sh.comm_stream);
        }
        out->small_collectives = mm->shards[0].pc.connected ? 2 : mm->tp == 1 ? 0 : mm->tp_mode == FL_TP_EMULATED ? 3 : 1;
        out->fused_all_reduce = fused_all_reduce_ready(mm) ? 1 : 0;
        if (mm->shards[0].comm) {
            int n = 0;
            if (ncclCommCount(mm->shards[0].comm, &n) == ncclSuccess) out->rccl_ranks = n;
        }
        return FL_OK;
    });
}

int fl_cache_create(fl_model *m, size_t max_seq, fl_cache **out) {
    return guarded([&]() -> int {
        if (!out) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_cache_create: null out");
        *out = nullptr;
        Cache *c = nullptr;
        int rc = cache_create(M(m), max_seq, &c);
        if (rc == FL_OK) *out = reinterpret_cast<fl_cache *>(c);
        return rc;
    });
}
void fl_cache_reset(fl_cache *c) {
    guarded_void([&]() {
        if (c) C(c)->len = 0;
    });
}
size_t fl_cache_len(const fl_cache *c) { return c ? C(c)->len : 0; }
size_t fl_cache_capacity(const fl_cache *c) { return c ? C(c)->max_seq : 0; }
void fl_cache_destroy(fl_cache *c) {
    guarded_void([&]() {
        if (!c) return;
        Model *m = C(c)->m;
        delete C(c);
        if (m && m->refs.fetch_sub(1) == 1) delete m;
    });
}

int fl_forward(fl_model *m, fl_cache *c, const uint32_t *ids, size_t T, size_t pos, float *logits_out) {
    return guarded([&]() -> int {
        if (!logits_out) FL_FAIL(FL_ERR_BAD_ARGUMENT, "null logits_out");
        return forward(M(m), C(c), ids, T, pos, logits_out, nullptr);
    });
}

int fl_cache_truncate(fl_cache *c, size_t len) {
    return guarded([&]() -> int {
        return cache_truncate(C(c), len);
    });
}

int fl_cache_copy_prefix(fl_cache *dst, const fl_cache *src, size_t n) {
    return guarded([&]() -> int {
        return cache_copy_prefix(C(dst), C(src), n);
    });
}

int fl_forward_verify(fl_model *m, fl_cache *c, uint32_t token, const uint32_t *draft, size_t n_draft, size_t pos, uint32_t *tokens_out,
                      size_t *n_out, float *logits_out) {
    return guarded([&]() -> int {
        return forward_verify(M(m), C(c), token, draft, n_draft, pos, tokens_out, n_out, logits_out);
    });
}

int fl_lookup_draft(const uint32_t *history, size_t n_history, const fl_lookup *opts, size_t limit, uint32_t *draft_out, size_t *n_draft_out) {
    return guarded([&]() -> int {
        if (n_draft_out) *n_draft_out = 0;
        FL_TRY(check_lookup(opts));
        if (!n_draft_out || (n_history && !history) || (limit && !draft_out)) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_lookup_draft: null argument");
        *n_draft_out = lookup_draft(history, n_history, opts->max_draft, opts->ngram_max, opts->ngram_min, limit, draft_out);
        return FL_OK;
    });
}

int fl_decode_lookup(fl_model *m, fl_cache *c, const uint32_t *corpus, size_t n_corpus, uint32_t first_token, size_t pos, size_t n_steps,
                     int64_t eos, const fl_lookup *opts, uint32_t *tokens_out, size_t *n_out, fl_spec_stats *stats) {
    return guarded([&]() -> int {
        return decode_lookup(M(m), C(c), corpus, n_corpus, first_token, pos, n_steps, eos, opts, tokens_out, n_out, stats);
    });
}

int fl_forward_verify_ex(fl_model *m, fl_cache *c, uint32_t token, const uint32_t *draft, size_t n_draft, size_t pos, const fl_sampler *sampler,
                         uint32_t *tokens_out, size_t *n_out, float *logits_out) {
    return guarded([&]() -> int {
        return forward_verify(M(m), C(c), token, draft, n_draft, pos, tokens_out, n_out, logits_out, sampler);
    });
}

int fl_decode_lookup_ex(fl_model *m, fl_cache *c, const uint32_t *corpus, size_t n_corpus, uint32_t first_token, size_t pos, size_t n_steps,
                        int64_t eos, const fl_lookup *opts, const fl_sampler *sampler, uint32_t *tokens_out, size_t *n_out, fl_spec_stats *stats) {
    return guarded([&]() -> int {
        return decode_lookup(M(m), C(c), corpus, n_corpus, first_token, pos, n_steps, eos, opts, tokens_out, n_out, stats, sampler);
    });
}

int fl_forward_verify_lp(fl_model *m, fl_cache *c, uint32_t token, const uint32_t *draft, size_t n_draft, size_t pos, const fl_sampler *sampler,
                         const fl_logprobs *lp, uint32_t *tokens_out, size_t *n_out, float *logits_out) {
    return guarded([&]() -> int {
        return forward_verify_lp(M(m), C(c), token, draft, n_draft, pos, sampler, lp, tokens_out, n_out, logits_out);
    });
}

int fl_decode_lookup_lp(fl_model *m, fl_cache *c, const uint32_t *corpus, size_t n_corpus, uint32_t first_token, size_t pos, size_t n_steps,
                        int64_t eos, const fl_lookup *opts, const fl_sampler *sampler, const fl_logprobs *lp, uint32_t *tokens_out, size_t *n_out,
                        fl_spec_stats *stats) {
    return guarded([&]() -> int {
        return decode_lookup_lp(M(m), C(c), corpus, n_corpus, first_token, pos, n_steps, eos, opts, sampler, lp, tokens_out, n_out, stats);
    });
}

int fl_forward_argmax(fl_model *m, fl_cache *c, const uint32_t *ids, size_t T, size_t pos, uint32_t *token_out) {
    return guarded([&]() -> int {
        if (!token_out) FL_FAIL(FL_ERR_BAD_ARGUMENT, "null token_out");
        return forward(M(m), C(c), ids, T, pos, nullptr, token_out);
    });
}

int fl_decode_greedy(fl_model *m, fl_cache *c, uint32_t first_token, size_t pos, size_t n_steps, int64_t eos,
                     uint32_t *tokens_out, size_t *n_out) {
    return guarded([&]() -> int {
        return decode_greedy(M(m), C(c), first_token, pos, n_steps, eos, tokens_out, n_out);
    });
}

int fl_forward_sample_ex(fl_model *m, fl_cache *c, const uint32_t *ids, size_t T, size_t pos, const fl_sampler *sampler,
                         uint32_t *token_out) {
    return guarded([&]() -> int {
        if (!token_out || !sampler) FL_FAIL(FL_ERR_BAD_ARGUMENT, "null argument");
        return forward(M(m), C(c), ids, T, pos, nullptr, token_out, sampler);
    });
}

int fl_forward_sample(fl_model *m, fl_cache *c, const uint32_t *ids, size_t T, size_t pos, const fl_sampling *sampling,
                      uint32_t *token_out) {
    if (!sampling) return fl_forward_sample_ex(m, c, ids, T, pos, nullptr, token_out);
    const fl_sampler s = widen(*sampling);
    return fl_forward_sample_ex(m, c, ids, T, pos, &s, token_out);
}

int fl_decode_sample_ex(fl_model *m, fl_cache *c, uint32_t first_token, size_t pos, size_t n_steps, int64_t eos,
                        const fl_sampler *sampler, uint32_t *tokens_out, size_t *n_out) {
    return guarded([&]() -> int {
        if (!sampler) FL_FAIL(FL_ERR_BAD_ARGUMENT, "null sampling");
        return decode_greedy(M(m), C(c), first_token, pos, n_steps, eos, tokens_out, n_out, sampler);
    });
}

int fl_decode_sample(fl_model *m, fl_cache *c, uint32_t first_token, size_t pos, size_t n_steps, int64_t eos,
                     const fl_sampling *sampling, uint32_t *tokens_out, size_t *n_out) {
    if (!sampling) return fl_decode_sample_ex(m, c, first_token, pos, n_steps, eos, nullptr, tokens_out, n_out);
    const fl_sampler s = widen(*sampling);
    return fl_decode_sample_ex(m, c, first_token, pos, n_steps, eos, &s, tokens_out, n_out);
}

// ---- token log-probabilities: the sampled entry points with an fl_logprobs (its errors come first: they need neither model nor device)
int fl_forward_sample_lp(fl_model *m, fl_cache *c, const uint32_t *ids, size_t T, size_t pos, const fl_sampler *sampler,
                         uint32_t *token_out, const fl_logprobs *lp) {
    return guarded([&]() -> int {
        FL_TRY(check_logprobs(lp, 0));
        if (!token_out) FL_FAIL(FL_ERR_BAD_ARGUMENT, "null token_out");
        return forward(M(m), C(c), ids, T, pos, nullptr, token_out, sampler, lp);
    });
}

int fl_decode_sample_lp(fl_model *m, fl_cache *c, uint32_t first_token, size_t pos, size_t n_steps, int64_t eos,
                        const fl_sampler *sampler, uint32_t *tokens_out, size_t *n_out, const fl_logprobs *lp) {
    return guarded([&]() -> int {
        FL_TRY(check_logprobs(lp, 0));
        return decode_greedy(M(m), C(c), first_token, pos, n_steps, eos, tokens_out, n_out, sampler, lp);
    });
}

int fl_batch_decode_each_lp(fl_batch *b, const uint32_t *first_tokens, const size_t *pos, size_t n_steps, const int64_t *eos,
                            const fl_sampler *samplers, uint32_t *tokens_out, size_t *n_out, const fl_logprobs *lp) {
    return guarded([&]() -> int {
        if (!lp) FL_FAIL(FL_ERR_BAD_ARGUMENT, "null fl_logprobs (lp)");
        return batch_decode_each(reinterpret_cast<Batch *>(b), first_tokens, pos, n_steps, eos, samplers, tokens_out, n_out, lp);
    });
}

// ---- prompt log-probabilities: the fl_score's own errors come first (they need neither model nor device)
int fl_forward_score(fl_model *m, fl_cache *c, const uint32_t *ids, size_t T, size_t pos, const fl_score *sc) {
    return guarded([&]() -> int {
        return forward_score(M(m), C(c), ids, T, pos, sc);
    });
}

int fl_batch_score(fl_model *m, fl_cache *const *caches, size_t n, const uint32_t *ids, const size_t *offsets, const size_t *pos, const fl_score *sc) {
    return guarded([&]() -> int {
        return batch_score(M(m), reinterpret_cast<Cache *const *>(caches), n, ids, offsets, pos, sc);
    });
}

// ---- logit rules: every argument error is decided before the model, the cache or the device is looked at
int fl_cache_set_logit_rules(fl_model *m, fl_cache *c, const fl_logit_rules *rules, const uint32_t *prompt_ids, size_t n_prompt,
                             const uint32_t *output_ids, size_t n_output) {
    return guarded([&]() -> int {
        return cache_set_logit_rules(M(m), C(c), rules, prompt_ids, n_prompt, output_ids, n_output);
    });
}

int fl_cache_logit_counts(fl_model *m, fl_cache *c, uint32_t *words_out) {
    return guarded([&]() -> int {
        return cache_logit_counts(M(m), C(c), words_out);
    });
}

// ---- guided decoding: the automaton's argument errors are decided before the model or the device is looked at
int fl_guide_create(fl_model *m, const fl_guide_desc *desc, fl_guide **out) {
    return guarded([&]() -> int {
        if (!out) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_guide_create: null out");
        *out = nullptr;
        Guide *g = nullptr;
        FL_TRY(guide_create(M(m), desc, &g));
        *out = reinterpret_cast<fl_guide *>(g);
        return FL_OK;
    });
}

void fl_guide_destroy(fl_guide *g) {
    guarded_void([&]() {
        guide_release(reinterpret_cast<Guide *>(g));
    });
}

int fl_cache_set_guide(fl_model *m, fl_cache *c, fl_guide *g, uint32_t state) {
    return guarded([&]() -> int {
        return cache_set_guide(M(m), C(c), reinterpret_cast<Guide *>(g), state);
    });
}

int fl_cache_guide_state(const fl_cache *c, uint32_t *state_out) {
    return guarded([&]() -> int {
        return cache_guide_state(C(c), state_out);
    });
}

int fl_batch_create(fl_model *m, fl_cache *const *caches, size_t n, fl_batch **out) {
    return guarded([&]() -> int {
        if (!out) FL_FAIL(FL_ERR_BAD_ARGUMENT, "null out");
        Batch *b = nullptr;
        FL_TRY(batch_create(M(m), reinterpret_cast<Cache *const *>(caches), n, &b));
        *out = reinterpret_cast<fl_batch *>(b);
        return FL_OK;
    });
}
void fl_batch_destroy(fl_batch *b) {
    guarded_void([&]() {
        if (!b) return;
        Batch *bb = reinterpret_cast<Batch *>(b);
        Model *m = bb->m;
        delete bb;
        if (m && m->refs.fetch_sub(1) == 1) delete m;
    });
}
int fl_batch_replace(fl_batch *b, size_t slot, fl_cache *cache) {
    return guarded([&]() -> int {
        return batch_replace(reinterpret_cast<Batch *>(b), slot, reinterpret_cast<Cache *>(cache));
    });
}
int fl_batch_forward(fl_batch *b, const uint32_t *tokens, const size_t *pos, float *logits_out, uint32_t *argmax_out) {
    return guarded([&]() -> int {
        return batch_forward(reinterpret_cast<Batch *>(b), tokens, pos, logits_out, argmax_out);
    });
}
int fl_batch_prefill(fl_model *m, fl_cache *const *caches, size_t n, const uint32_t *ids, const size_t *offsets, const size_t *pos,
                     const fl_sampler *samplers, uint32_t *tokens_out, float *logits_out) {
    return guarded([&]() -> int {
        return batch_prefill(M(m), reinterpret_cast<Cache *const *>(caches), n, ids, offsets, pos, samplers, tokens_out, logits_out);
    });
}
int fl_batch_verify(fl_model *m, fl_cache *const *caches, size_t n, const uint32_t *ids, const size_t *offsets, const size_t *pos,
                    const fl_sampler *samplers, uint32_t *tokens_out, size_t *n_out, float *logits_out) {
    return guarded([&]() -> int {
        return batch_verify(M(m), reinterpret_cast<Cache *const *>(caches), n, ids, offsets, pos, samplers, tokens_out, n_out, logits_out);
    });
}
int fl_batch_embed(fl_model *m, fl_cache *const *caches, size_t n, const uint32_t *ids, const size_t *offsets, const size_t *pos,
                   const fl_embed *opts, float *out) {
    return guarded([&]() -> int {
        return batch_embed(M(m), reinterpret_cast<Cache *const *>(caches), n, ids, offsets, pos, opts, out);
    });
}
int fl_batch_decode_lookup(fl_model *m, fl_cache *const *caches, size_t n, const uint32_t *corpus, const size_t *corpus_offsets,
                           const uint32_t *first_tokens, const size_t *pos, const size_t *n_steps, const int64_t *eos, const fl_lookup *opts,
                           const fl_sampler *samplers, uint32_t *tokens_out, size_t *n_out, fl_spec_stats *stats) {
    return guarded([&]() -> int {
        return batch_decode_lookup(M(m), reinterpret_cast<Cache *const *>(caches), n, corpus, corpus_offsets, first_tokens, pos, n_steps, eos, opts,
                                   samplers, tokens_out, n_out, stats);
    });
}
int fl_batch_decode(fl_batch *b, const uint32_t *first_tokens, const size_t *pos, size_t n_steps, int64_t eos,
                    const fl_sampling *sampling, uint32_t *tokens_out, size_t *n_out) {
    return guarded([&]() -> int {
        fl_sampler s{};
        if (sampling) s = widen(*sampling);
        return batch_decode(reinterpret_cast<Batch *>(b), first_tokens, pos, n_steps, eos, sampling ? &s : nullptr, tokens_out, n_out);
    });
}
int fl_batch_decode_each_ex(fl_batch *b, const uint32_t *first_tokens, const size_t *pos, size_t n_steps, const int64_t *eos,
                            const fl_sampler *samplers, uint32_t *tokens_out, size_t *n_out) {
    return guarded([&]() -> int {
        return batch_decode_each(reinterpret_cast<Batch *>(b), first_tokens, pos, n_steps, eos, samplers, tokens_out, n_out);
    });
}
int fl_batch_decode_each(fl_batch *b, const uint32_t *first_tokens, const size_t *pos, size_t n_steps, const int64_t *eos,
                         const fl_sampling *sampling, uint32_t *tokens_out, size_t *n_out) {
    return guarded([&]() -> int {
        if (!b) FL_FAIL(FL_ERR_BAD_ARGUMENT, "null argument");
        std::vector<fl_sampler> sp;
        if (sampling) for (int i = 0; i < reinterpret_cast<Batch *>(b)->B; i++) sp.push_back(widen(sampling[i]));
        return batch_decode_each(reinterpret_cast<Batch *>(b), first_tokens, pos, n_steps, eos, sampling ? sp.data() : nullptr, tokens_out, n_out);
    });
}

int fl_synchronize(fl_model *m) {
    return guarded([&]() -> int {
        if (!m) FL_FAIL(FL_ERR_BAD_ARGUMENT, "null model");
        for (auto &sh : M(m)->shards) { FL_HIP(hipSetDevice(sh.device)); FL_HIP(hipStreamSynchronize(sh.stream)); }
        return FL_OK;
    });
}

// ---- embeddings: the BERT / MiniLM encoder (encoder.hip) --------------------------------------------------------------------------
int fl_encoder_create(const fl_encoder_config *cfg, const fl_tensor *tensors, size_t n_tensors, int32_t compute_dtype, int32_t device,
                      fl_encoder **out) {
    return guarded([&]() -> int {
        if (!out) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_encoder_create: null out");
        *out = nullptr;
        Encoder *e = nullptr;
        const int rc = encoder_create(cfg, tensors, n_tensors, compute_dtype, device, &e);
        if (rc == FL_OK) *out = reinterpret_cast<fl_encoder *>(e);
        return rc;
    });
}
void fl_encoder_release(fl_encoder *e) {
    guarded_void([&]() { delete reinterpret_cast<Encoder *>(e); });
}
int fl_encoder_hidden(fl_encoder *e, const uint32_t *ids, size_t T, float *out) {
    return guarded([&]() -> int {
        if (!out) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_encoder_hidden: null out");
        const size_t offsets[2] = {0, T};
        return encoder_run(reinterpret_cast<Encoder *>(e), ids, offsets, 1, out, nullptr);
    });
}
int fl_encoder_embed(fl_encoder *e, const uint32_t *ids, const size_t *offsets, size_t n_seq, float *out) {
    return guarded([&]() -> int {
        if (!out) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_encoder_embed: null out");
        return encoder_run(reinterpret_cast<Encoder *>(e), ids, offsets, n_seq, nullptr, out);
    });
}

int fl_comm_probe(fl_model *m, int32_t form, int64_t n, int32_t iters, double *us_per_call) {
    return guarded([&]() -> int {
        if (!m) FL_FAIL(FL_ERR_BAD_ARGUMENT, "null model");
        return comm_probe(M(m), form, n, iters, us_per_call);
    });
}

int fl_comm_selftest(fl_model *m, int64_t n, int32_t *ok) {
    return guarded([&]() -> int {
        if (!m || !ok) FL_FAIL(FL_ERR_BAD_ARGUMENT, "null argument");
        int good = 0;
        const int rc = comm_selftest(M(m), n, &good);
        *ok = good;
        return rc;
    });
}

int fl_tp_slice(const fl_config *cfg, const char *tensor_name, int32_t tp_rank, int32_t tp_size, int64_t out[4]) {
    return guarded([&]() -> int {
        if (!tensor_name || !out) FL_FAIL(FL_ERR_BAD_ARGUMENT, "null argument");
        Dims D;
        FL_TRY(resolve_config(cfg, &D));
        return tp_slice(D, tensor_name, tp_rank, tp_size, out);
    });
}

int fl_profile_begin(fl_model *m) {
    return guarded([&]() -> int {
        if (!m) FL_FAIL(FL_ERR_BAD_ARGUMENT, "null model");
        std::lock_guard<std::mutex> lock(M(m)->mu);
        for (auto &r : M(m)->prof) { (void)hipEventDestroy(r.e0); (void)hipEventDestroy(r.e1); }
        M(m)->prof.clear();
        M(m)->profiling = true;
        return FL_OK;
    });
}

int fl_profile_end(fl_model *m, fl_kernel_stat *stats, size_t cap, size_t *n_stats) {
    return guarded([&]() -> int {
        if (!m || !n_stats) FL_FAIL(FL_ERR_BAD_ARGUMENT, "null argument");
        Model *mm = M(m);
        std::lock_guard<std::mutex> lock(mm->mu);
        mm->profiling = false;
        for (auto &sh : mm->shards) { FL_HIP(hipSetDevice(sh.device)); FL_HIP(hipStreamSynchronize(sh.stream)); }
        std::vector<fl_kernel_stat> acc;
        for (auto &r : mm->prof) {
            float ms = 0.f;
            FL_HIP(hipEventElapsedTime(&ms, r.e0, r.e1));
            char name[48];
            if (r.tag[0]) snprintf(name, sizeof name, "%s[%s]", kernel_class_name(r.kc), r.tag);
            else snprintf(name, sizeof name, "%s", kernel_class_name(r.kc));
            fl_kernel_stat *st = nullptr;
            for (auto &e : acc) if (!strcmp(e.name, name)) { st = &e; break; }
            if (!st) { fl_kernel_stat e; memset(&e, 0, sizeof e); snprintf(e.name, sizeof e.name, "%s", name); acc.push_back(e); st = &acc.back(); }
            st->launches++; st->total_ms += ms; st->bytes += r.bytes; st->flops += r.flops;
        }
        for (auto &r : mm->prof) { (void)hipEventDestroy(r.e0); (void)hipEventDestroy(r.e1); }
        mm->prof.clear();
        size_t n = 0;
        for (auto &e : acc) {
            if (stats && n < cap) stats[n] = e;
            n++;
        }
        *n_stats = n;
        return FL_OK;
    });
}

int fl_tune(const char *key, int value) {
    return guarded([&]() -> int {
        if (!key || value < -1) FL_FAIL(FL_ERR_BAD_ARGUMENT, "bad tuning key/value");       // (-1: "automatic", for the switches that have it)
        if (!strcmp(key, "gemv_blocks")) gemv_set_tuning(value, -1);                    // 0 = automatic
        else if (!strcmp(key, "gemv_waves")) gemv_set_tuning(-1, value);                // 0 = automatic
        else if (!strcmp(key, "engine_grid")) {                                         // 0 = one workgroup per CU (tests: a grid that cannot be resident)
#ifndef FL_EXPERIMENTAL
            FL_FAIL(FL_ERR_UNSUPPORTED, "default build: engine_grid belongs to the experimental decode engine");
#endif
            engine_set_grid(value);
        }
        else if (!strcmp(key, "experimental")) {                                        // is this the EXPERIMENTAL build? (tests skip otherwise)
#ifndef FL_EXPERIMENTAL
            FL_FAIL(FL_ERR_UNSUPPORTED, "default build: the experimental kernels (decode engine, fused attention + o_proj, attention prefetch, loader waves) are not compiled in");
#endif
        }
        else if (!strcmp(key, "reload_env")) tune_reload_env();                        // re-read every FL_<NAME> switch of the table (common.h)
        else {
            const int rc = tune_set(key, value);
            if (rc == FL_ERR_UNSUPPORTED) FL_FAIL(FL_ERR_UNSUPPORTED, "default build: %s is a switch of a kernel compiled into the EXPERIMENTAL build only", key);
            if (rc != FL_OK) FL_FAIL(FL_ERR_BAD_ARGUMENT, "unknown tuning key %s", key);
        }
        return FL_OK;
    });
}

}  // extern "C"

