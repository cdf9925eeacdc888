// api.hip -- the extern "C" surface declared in include/fastllm_mi355x.h.
//
// Every entry point is an exception barrier: the host of this library is Rust (or ctypes), and a C++
// exception that crosses the C ABI is undefined behaviour there.  The reference surfaces failures as
// anyhow::Error (mod.rs:402-405,446-451); here std::bad_alloc becomes FL_ERR_OOM and anything else
// FL_ERR_HIP, both with fl_last_error() set.
#include <algorithm>
#include <exception>
#include <memory>
#include <new>
#include <vector>

#include "model.h"
#include "encoder.h"
#include "lookup.h"

using namespace fl;

// fl_model / fl_cache stay opaque: the handles are the C++ objects themselves

static Model *M(fl_model *m) { return reinterpret_cast<Model *>(m); }
static const Model *M(const fl_model *m) { return reinterpret_cast<const Model *>(m); }
static Cache *C(fl_cache *c) { return reinterpret_cast<Cache *>(c); }
static const Cache *C(const fl_cache *c) { return reinterpret_cast<const Cache *>(c); }

template <typename F> static int guarded(F &&body) noexcept {
    try {
        return body();
    } catch (const std::bad_alloc &) {
        set_error("out of host memory (std::bad_alloc)");
        return FL_ERR_OOM;
    } catch (const std::exception &e) {
        set_error("internal error: %s", e.what());
        return FL_ERR_HIP;
    } catch (...) {
        set_error("internal error: unknown C++ exception");
        return FL_ERR_HIP;
    }
}
template <typename F> static void guarded_void(F &&body) noexcept {
    (void)guarded([&]() -> int { body(); return FL_OK; });
}

// ---- fl_op_attention_plain / fl_op_attention_batch: the attention launches on caches built here in the model's layout ----------
namespace {

struct AttnOpBufs {
    std::vector<void *> p; hipStream_t s = 0;
    ~AttnOpBufs() { if (s) (void)hipStreamSynchronize(s);
                    for (void *x : p) (void)hipFree(x);
                    if (s) (void)hipStreamDestroy(s); }
    int alloc(void **out, size_t bytes) { *out = nullptr; FL_HIP(hipMalloc(out, bytes ? bytes : 4)); p.push_back(*out); return FL_OK; }
    int upload(void **out, const void *src, size_t bytes) { FL_TRY(alloc(out, bytes)); FL_HIP(hipMemcpy(*out, src, bytes, hipMemcpyHostToDevice)); return FL_OK; }
};

// One sequence's K and V as cache_create lays them out: K [L][Hkv][sa][d]; V the same, or transposed [L][Hkv][d][sa] for the MFMA
// kernels.  Host rows [L][rows][Hkv*d]; every position >= rows holds `pad`.  E: the element's bit pattern (uint16_t / uint32_t).
template <typename E>
void attn_op_cache(std::vector<E> &kc, std::vector<E> &vc, const void *k, const void *v, int64_t L, int64_t rows, int64_t Hkv, int64_t sa,
                   int64_t d, bool v_transposed, E pad) {
    kc.assign((size_t)(L * Hkv * sa * d), pad); vc.assign((size_t)(L * Hkv * sa * d), pad);
    const E *kh = reinterpret_cast<const E *>(k), *vh = reinterpret_cast<const E *>(v);
    for (int64_t l = 0; l < L; l++)
        for (int64_t s = 0; s < rows; s++)
            for (int64_t h = 0; h < Hkv; h++)
                for (int64_t j = 0; j < d; j++) {
                    const size_t src = (size_t)(((l * rows + s) * Hkv + h) * d + j), head = (size_t)((l * Hkv + h) * sa * d);
                    kc[head + (size_t)(s * d + j)] = kh[src];
                    vc[head + (size_t)(v_transposed ? j * sa + s : s * d + j)] = vh[src];
                }
}

int attn_op_upload_cache(AttnOpBufs &B, void **kd, void **vd, int32_t dtype, const void *k, const void *v, int64_t L, int64_t rows, int64_t Hkv,
                         int64_t sa, int64_t d, bool v_transposed, float pad_value) {
    if (dtype == FL_DTYPE_BF16) {
        std::vector<uint16_t> kc, vc;
        attn_op_cache<uint16_t>(kc, vc, k, v, L, rows, Hkv, sa, d, v_transposed, float_to_bf16_bits_host(pad_value));
        FL_TRY(B.upload(kd, kc.data(), kc.size() * 2)); FL_TRY(B.upload(vd, vc.data(), vc.size() * 2));
    } else {
        union { float f; uint32_t u; } pv; pv.f = pad_value;
        std::vector<uint32_t> kc, vc;
        attn_op_cache<uint32_t>(kc, vc, k, v, L, rows, Hkv, sa, d, v_transposed, pv.u);
        FL_TRY(B.upload(kd, kc.data(), kc.size() * 4)); FL_TRY(B.upload(vd, vc.data(), vc.size() * 4));
    }
    return FL_OK;
}

// the split scratch of one cache, sized as cache_create sizes it
int attn_op_scratch(AttnOpBufs &B, float **pm, float **pl, float **po, unsigned **cnt, int64_t H, int64_t d, int nsplit) {
    FL_TRY(B.alloc((void **)pm, (size_t)H * nsplit * 4)); FL_TRY(B.alloc((void **)pl, (size_t)H * nsplit * 4));
    FL_TRY(B.alloc((void **)po, (size_t)H * nsplit * d * 4)); FL_TRY(B.alloc((void **)cnt, (size_t)H * 4));
    FL_HIP(hipMemset(*cnt, 0, (size_t)H * 4));
    return FL_OK;
}

// the launches' outputs, [n] elements of `dtype` on the device, widened to fp32
int attn_op_download(float *out, const void *dev, size_t n, int32_t dtype) {
    if (dtype == FL_DTYPE_BF16) {
        std::vector<bf16_t> oh(n);
        FL_HIP(hipMemcpy(oh.data(), dev, n * 2, hipMemcpyDeviceToHost));
        for (size_t i = 0; i < n; i++) out[i] = bf16_bits_to_float(oh[i]);
    } else {
        FL_HIP(hipMemcpy(out, dev, n * 4, hipMemcpyDeviceToHost));
    }
    return FL_OK;
}

int attn_op_check_heads(int32_t dtype, int32_t layout, int64_t H, int64_t Hkv, int64_t d) {
    if ((dtype != FL_DTYPE_BF16 && dtype != FL_DTYPE_F32) || layout < 0 || layout > 1) FL_FAIL(FL_ERR_BAD_ARGUMENT, "dtype: bf16 or f32; layout: 0 plain, 1 MFMA");
    if (H < 1 || Hkv < 1 || H % Hkv != 0) FL_FAIL(FL_ERR_BAD_ARGUMENT, "bad head counts (H a multiple of Hkv)");
    if (d != 64 && d != 128) FL_FAIL(FL_ERR_UNSUPPORTED, "attention: head_dim %lld not supported (64 or 128)", (long long)d);
    if (layout == 1 && !attn_mfma_supported(dtype, H, Hkv, d)) FL_FAIL(FL_ERR_UNSUPPORTED, "MFMA attention: bf16, head_dim 64 / 128, at most 8 query heads per kv head");
    return FL_OK;
}

}  // namespace

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

int fl_op_verify_select(const float *logits, int64_t T, int64_t V, const uint32_t *draft, uint32_t *argmax_out, int64_t *n_accepted_out) {
    return guarded([&]() -> int {
        if (!logits || !argmax_out || !n_accepted_out) FL_FAIL(FL_ERR_BAD_ARGUMENT, "null argument");
        if (T < 1 || T > kVerifyMaxRows || V <= 0 || V > (1 << 24)) FL_FAIL(FL_ERR_BAD_ARGUMENT, "bad size (1 <= T <= %d)", kVerifyMaxRows);
        if (T > 1 && !draft) FL_FAIL(FL_ERR_BAD_ARGUMENT, "null draft");
        int ndev = 0;
        if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) FL_FAIL(FL_ERR_NO_DEVICE, "no HIP device visible: this library has no CPU path");
        FL_HIP(hipSetDevice(0));
        struct Bufs { float *lg = 0; uint32_t *dr = 0, *out = 0; hipStream_t s = 0;
                      ~Bufs() { (void)hipFree(lg); (void)hipFree(dr); (void)hipFree(out); if (s) (void)hipStreamDestroy(s); } } B;
        FL_HIP(hipStreamCreate(&B.s));
        FL_HIP(hipMalloc((void **)&B.lg, (size_t)T * V * 4));
        FL_HIP(hipMalloc((void **)&B.dr, (size_t)kVerifyMaxRows * 4));
        FL_HIP(hipMalloc((void **)&B.out, (size_t)kVerifyWords * 4));
        FL_HIP(hipMemcpy(B.lg, logits, (size_t)T * V * 4, hipMemcpyHostToDevice));
        if (T > 1) FL_HIP(hipMemcpy(B.dr, draft, (size_t)(T - 1) * 4, hipMemcpyHostToDevice));
        FL_HIP(hipMemset(B.out, 0, (size_t)kVerifyWords * 4));
        Launcher L; L.stream = B.s;
        uint32_t host[2][kVerifyWords];
        for (int rep = 0; rep < 2; rep++) {                     // twice: the second launch meets the ticket word the first one put back
            FL_TRY(launch_verify_select(L, B.lg, V, (int)T, B.dr, B.out));
            FL_HIP(hipStreamSynchronize(B.s));
            FL_HIP(hipMemcpy(host[rep], B.out, sizeof host[rep], hipMemcpyDeviceToHost));
        }
        if (memcmp(host[0], host[1], sizeof host[0]) || host[1][kVerifyTicket] != 0)
            FL_FAIL(FL_ERR_HIP, "verify_select: a repeated launch gave another result (ticket %u)", host[1][kVerifyTicket]);
        for (int64_t t = 0; t < T; t++) argmax_out[t] = host[0][t];
        *n_accepted_out = (int64_t)host[0][kVerifyNacc];
        return FL_OK;
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

// the older sampler struct as the one every path below takes: no top_p, no top_k
static fl_sampler widen(const fl_sampling &sp) {
    fl_sampler s{};
    s.struct_size = sizeof(fl_sampler);
    s.temperature = sp.temperature; s.seed = sp.seed; s.draws_done = sp.draws_done;
    return s;
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

int fl_op_logprobs(const float *logits, int64_t T, int64_t V, const uint32_t *chosen, int32_t top_n, float *token_logprob,
                   uint32_t *top_ids, float *top_logprobs) {
    return guarded([&]() -> int {
        if (!logits || !chosen || !token_logprob) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_op_logprobs: null logits, chosen or token_logprob");
        if (T < 1 || T > 64) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_op_logprobs: T %lld not in 1..64", (long long)T);
        if (V < 1 || V > (1 << 24)) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_op_logprobs: V %lld not in 1..2^24", (long long)V);
        if (top_n < 0 || top_n > FL_LOGPROBS_MAX_TOP || top_n > V)
            FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_op_logprobs: top_n %d not in 0..min(%d, V = %lld)", top_n, FL_LOGPROBS_MAX_TOP, (long long)V);
        if (top_n > 0 && (!top_ids || !top_logprobs)) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_op_logprobs: null top_ids or top_logprobs with top_n %d", top_n);
        for (int64_t t = 0; t < T; t++)
            if ((int64_t)chosen[t] >= V) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_op_logprobs: chosen[%lld] = %u is not below V = %lld", (long long)t, chosen[t], (long long)V);
        int ndev = 0;
        if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) FL_FAIL(FL_ERR_NO_DEVICE, "no HIP device visible: this library has no CPU path");
        FL_HIP(hipSetDevice(0));
        struct Bufs { float *lg = 0; uint32_t *ch = 0; LogprobRec *recs = 0; LogprobCtl *ctl = 0; hipStream_t s = 0;
                      ~Bufs() { (void)hipFree(lg); (void)hipFree(ch); (void)hipFree(recs); (void)hipFree(ctl); if (s) (void)hipStreamDestroy(s); } } B;
        FL_HIP(hipStreamCreate(&B.s));
        FL_HIP(hipMalloc((void **)&B.lg, (size_t)T * V * 4));
        FL_HIP(hipMalloc((void **)&B.ch, (size_t)T * 4));
        FL_HIP(hipMalloc((void **)&B.recs, (size_t)T * sizeof(LogprobRec)));
        FL_HIP(hipMalloc((void **)&B.ctl, sizeof(LogprobCtl)));
        FL_HIP(hipMemcpy(B.lg, logits, (size_t)T * V * 4, hipMemcpyHostToDevice));
        FL_HIP(hipMemcpy(B.ch, chosen, (size_t)T * 4, hipMemcpyHostToDevice));
        Launcher L; L.stream = B.s;
        FL_TRY(launch_set_logprob_ctl(L, B.ctl, B.recs, (uint32_t)T, top_n));
        LogprobSrc src;
        src.ctl = B.ctl; src.chosen = B.ch;
        std::vector<LogprobRec> host[2];
        for (int rep = 0; rep < 2; rep++) {                     // twice: the gather's order in LDS differs from launch to launch, the result must not
            host[rep].resize((size_t)T);
            FL_HIP(hipMemsetAsync(B.recs, 0, (size_t)T * sizeof(LogprobRec), B.s));
            FL_TRY(launch_token_logprobs(L, B.lg, V, (int)T, src, 0));
            FL_HIP(hipStreamSynchronize(B.s));
            FL_HIP(hipMemcpy(host[rep].data(), B.recs, (size_t)T * sizeof(LogprobRec), hipMemcpyDeviceToHost));
        }
        if (memcmp(host[0].data(), host[1].data(), (size_t)T * sizeof(LogprobRec))) FL_FAIL(FL_ERR_HIP, "token_logprobs: a repeated launch gave another result");
        for (int64_t t = 0; t < T; t++) {
            token_logprob[t] = host[0][(size_t)t].chosen;
            for (int j = 0; j < top_n; j++) {
                top_ids[t * top_n + j] = host[0][(size_t)t].ids[j];
                top_logprobs[t * top_n + j] = host[0][(size_t)t].lps[j];
            }
        }
        return FL_OK;
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

int fl_op_encoder_attention(const void *q, const void *k, const void *v, const size_t *offsets, size_t n_seq, int64_t H, int64_t d,
                            int32_t dtype, float *out) {
    return guarded([&]() -> int {
        if (!q || !k || !v || !out) FL_FAIL(FL_ERR_BAD_ARGUMENT, "null argument");
        if (dtype != FL_DTYPE_BF16 && dtype != FL_DTYPE_F32) FL_FAIL(FL_ERR_BAD_ARGUMENT, "dtype must be bf16 or f32");
        if (H < 1 || H > 65535) FL_FAIL(FL_ERR_BAD_ARGUMENT, "bad head count");
        if (!encoder_attention_supported(d)) FL_FAIL(FL_ERR_UNSUPPORTED, "encoder attention: head_dim 32 or 64");
        int64_t T = 0, longest = 0;
        FL_TRY(encoder_check_offsets(offsets, n_seq, 1 << 18, 1 << 20, &T, &longest));
        int ndev = 0;
        if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) FL_FAIL(FL_ERR_NO_DEVICE, "no HIP device visible: this library has no CPU path");
        FL_HIP(hipSetDevice(0));
        const size_t es = dtype == FL_DTYPE_BF16 ? 2 : 4, n = (size_t)T * H * d;
        struct Bufs { void *q = 0, *k = 0, *v = 0, *o = 0; int32_t *off = 0; hipStream_t s = 0;
                      ~Bufs() { (void)hipFree(q); (void)hipFree(k); (void)hipFree(v); (void)hipFree(o); (void)hipFree(off); if (s) (void)hipStreamDestroy(s); } } B;
        std::vector<int32_t> off(n_seq + 1);
        for (size_t s = 0; s <= n_seq; s++) off[s] = (int32_t)offsets[s];
        FL_HIP(hipStreamCreate(&B.s));
        FL_HIP(hipMalloc(&B.q, n * es)); FL_HIP(hipMalloc(&B.k, n * es)); FL_HIP(hipMalloc(&B.v, n * es)); FL_HIP(hipMalloc(&B.o, n * es));
        FL_HIP(hipMalloc((void **)&B.off, (n_seq + 1) * 4));
        FL_HIP(hipMemcpy(B.q, q, n * es, hipMemcpyHostToDevice));
        FL_HIP(hipMemcpy(B.k, k, n * es, hipMemcpyHostToDevice));
        FL_HIP(hipMemcpy(B.v, v, n * es, hipMemcpyHostToDevice));
        FL_HIP(hipMemcpy(B.off, off.data(), (n_seq + 1) * 4, hipMemcpyHostToDevice));
        FL_HIP(hipMemset(B.o, 0xff, n * es));                      // NaN pattern: an element the kernel does not write shows up
        Launcher L; L.stream = B.s;
        FL_TRY(launch_encoder_attention(L, dtype, B.q, B.k, B.v, H * d, B.off, (int64_t)n_seq, longest, T, H, d, 1.0f / sqrtf((float)d), B.o));
        FL_HIP(hipStreamSynchronize(B.s));
        if (dtype == FL_DTYPE_F32) {
            FL_HIP(hipMemcpy(out, B.o, n * 4, hipMemcpyDeviceToHost));
        } else {
            std::vector<bf16_t> oh(n);
            FL_HIP(hipMemcpy(oh.data(), B.o, n * 2, hipMemcpyDeviceToHost));
            for (size_t i = 0; i < n; i++) out[i] = bf16_bits_to_float(oh[i]);
        }
        return FL_OK;
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

int fl_op_sample_ex(const float *logits, int64_t V, const fl_sampler *sampler, int64_t n_draws, uint32_t *tokens_out, int64_t *kept_out) {
    return guarded([&]() -> int {
        if (!logits || !sampler || !tokens_out) FL_FAIL(FL_ERR_BAD_ARGUMENT, "null argument");
        if (V <= 0 || V > (1 << 24) || n_draws <= 0 || n_draws > (1 << 20)) FL_FAIL(FL_ERR_BAD_ARGUMENT, "bad size");
        SampleState ss;
        FL_TRY(make_sampler(sampler, V, &ss));
        int ndev = 0;
        if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) FL_FAIL(FL_ERR_NO_DEVICE, "no HIP device visible: this library has no CPU path");
        FL_HIP(hipSetDevice(0));
        struct Bufs { float *lg = 0, *sc = 0; StepState *st = 0; SampleState *ss = 0; uint32_t *out = 0, *kept = 0; hipStream_t s = 0;
                      ~Bufs() { (void)hipFree(lg); (void)hipFree(sc); (void)hipFree(st); (void)hipFree(ss); (void)hipFree(out); (void)hipFree(kept);
                                if (s) (void)hipStreamDestroy(s); } } B;
        const bool kept_dev = kept_out && ss.filter;       // (no filter: every token is kept)
        FL_HIP(hipStreamCreate(&B.s));
        FL_HIP(hipMalloc((void **)&B.lg, (size_t)V * 4));
        FL_HIP(hipMalloc((void **)&B.sc, (size_t)V * 4));
        FL_HIP(hipMalloc((void **)&B.st, sizeof(StepState)));
        FL_HIP(hipMalloc((void **)&B.ss, sizeof(SampleState)));
        FL_HIP(hipMalloc((void **)&B.out, (size_t)n_draws * 4));
        if (kept_dev) FL_HIP(hipMalloc((void **)&B.kept, (size_t)n_draws * 4));
        StepState st{}; st.eos = -1;
        FL_HIP(hipMemcpy(B.lg, logits, (size_t)V * 4, hipMemcpyHostToDevice));
        FL_HIP(hipMemcpy(B.st, &st, sizeof st, hipMemcpyHostToDevice));
        FL_HIP(hipMemcpy(B.ss, &ss, sizeof ss, hipMemcpyHostToDevice));
        Launcher L; L.stream = B.s;
        for (int64_t i = 0; i < n_draws; i++) {
            FL_TRY(launch_select_advance(L, B.lg, V, B.st, B.ss, B.sc, B.out, 1));
            if (kept_dev) FL_HIP(hipMemcpyAsync(B.kept + i, &B.ss->kept, 4, hipMemcpyDeviceToDevice, B.s));
        }
        FL_HIP(hipStreamSynchronize(B.s));
        FL_HIP(hipMemcpy(tokens_out, B.out, (size_t)n_draws * 4, hipMemcpyDeviceToHost));
        if (kept_out) {
            std::vector<uint32_t> k((size_t)n_draws, (uint32_t)V);
            if (kept_dev) FL_HIP(hipMemcpy(k.data(), B.kept, (size_t)n_draws * 4, hipMemcpyDeviceToHost));
            for (int64_t i = 0; i < n_draws; i++) kept_out[i] = (int64_t)k[(size_t)i];
        }
        return FL_OK;
    });
}

int fl_op_sample(const float *logits, int64_t V, const fl_sampling *sampling, int64_t n_draws, uint32_t *tokens_out) {
    if (!sampling) return fl_op_sample_ex(logits, V, nullptr, n_draws, tokens_out, nullptr);
    const fl_sampler s = widen(*sampling);
    return fl_op_sample_ex(logits, V, &s, n_draws, tokens_out, nullptr);
}

int fl_op_linear(const void *x, const void *w, const float *bias, int64_t T, int64_t N, int64_t K, int32_t dtype,
                 int32_t epilogue, float *y, int32_t iters, double *ms_out) {
    return guarded([&]() -> int {
        if (!x || !w || !y) FL_FAIL(FL_ERR_BAD_ARGUMENT, "null argument");
        if (dtype != FL_DTYPE_BF16 && dtype != FL_DTYPE_F32) FL_FAIL(FL_ERR_UNSUPPORTED, "dtype must be bf16 or f32");
        if (T <= 0 || N <= 0 || K <= 0 || K % 8) FL_FAIL(FL_ERR_BAD_ARGUMENT, "bad shape (K must be a multiple of 8)");
        if (epilogue == EPI_GATEUP && (N % 2)) FL_FAIL(FL_ERR_BAD_ARGUMENT, "gate/up needs an even row count");
        int ndev = 0;
        if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) FL_FAIL(FL_ERR_NO_DEVICE, "no HIP device visible: this library has no CPU path");
        FL_HIP(hipSetDevice(0));
        const size_t es = dtype == FL_DTYPE_BF16 ? 2 : 4;
        const int64_t I = N / 2, Ip = (I + 15) / 16 * 16;
        const int64_t Nw = epilogue == EPI_GATEUP ? 2 * Ip : N;          // rows of the device matrix
        const int64_t Ny = epilogue == EPI_GATEUP ? Ip : N;              // columns of the device output
        struct Bufs { void *x = 0, *w = 0, *ws = 0, *y = 0; float *b = 0; hipStream_t s = 0; hipEvent_t e0 = 0, e1 = 0;
                      std::vector<void *> copies;
                      ~Bufs() { (void)hipFree(x); (void)hipFree(w); (void)hipFree(ws); (void)hipFree(y); (void)hipFree(b);
                                for (size_t i = 1; i < copies.size(); i++) (void)hipFree(copies[i]);
                                if (s) { (void)hipStreamSynchronize(s); gemm_8p_release_stream(s); gemm_h4_release_stream(s); (void)hipStreamDestroy(s); }
                                if (e0) (void)hipEventDestroy(e0);
                                if (e1) (void)hipEventDestroy(e1); } } B;
        FL_HIP(hipStreamCreate(&B.s));
        FL_HIP(hipMalloc(&B.x, (size_t)T * K * es));
        FL_HIP(hipMalloc(&B.w, (size_t)Nw * K * es));
        const size_t ybytes = (size_t)T * Ny * (epilogue == EPI_GATEUP ? es : 4);
        const int op_split = tune(TK_OP_MAXSPLIT);
        const int max_split = (epilogue == EPI_F32 && !bias) ? (op_split > 0 ? op_split : std::max(4, ksplit_cap(T))) : 1;      // exercise split-K where the model would
        int nsplit = 1;
        FL_HIP(hipMalloc(&B.y, ybytes * max_split));
        FL_HIP(hipMemcpy(B.x, x, (size_t)T * K * es, hipMemcpyHostToDevice));
        Launcher L; L.stream = B.s;
        if (epilogue == EPI_GATEUP) {
            FL_HIP(hipMalloc(&B.ws, (size_t)N * K * es));
            FL_HIP(hipMemcpy(B.ws, w, (size_t)N * K * es, hipMemcpyHostToDevice));
            FL_HIP(hipMemsetAsync(B.w, 0, (size_t)Nw * K * es, B.s));
            FL_TRY(launch_convert_slice(L, dtype, B.ws, K, 0, 0, I, K, dtype, B.w, K, 0, 1));
            FL_TRY(launch_convert_slice(L, dtype, B.ws, K, I, 0, I, K, dtype, B.w, K, 0, 2));
        } else {
            FL_HIP(hipMemcpy(B.w, w, (size_t)N * K * es, hipMemcpyHostToDevice));
            if (bias) {
                FL_HIP(hipMalloc((void **)&B.b, (size_t)N * 4));
                FL_HIP(hipMemcpy(B.b, bias, (size_t)N * 4, hipMemcpyHostToDevice));
            }
        }
        // FL_OP_LINEAR_DMA=1: T <= 8 rows go through the batched-decode projection kernel (k_gemv_dma.hip) instead, so that
        // its weight-streaming rate can be measured (and its arithmetic tested) without a model around it
        const bool use_dma = tune(TK_OP_LINEAR_DMA) == 1;
        const bool dma = use_dma && dtype == FL_DTYPE_BF16 && T <= 32 && !B.b && gemv_dma_supported((int)T, Nw, K, epilogue, 0) &&
                         gemv_dma_ksplit(K, Nw, epilogue) <= max_split;
        auto run = [&](const void *wp) -> int {
            if (!dma) return launch_linear(L, dtype, wp, B.x, B.b, B.y, T, Nw, K, epilogue, nullptr, max_split, &nsplit);
            GemvBatchArgs ga;
            ga.W = wp; ga.x = B.x; ga.out = B.y; ga.N = (int)Nw; ga.K = (int)K; ga.epi = epilogue; ga.pro = PRO_X; ga.B = (int)T;
            ga.nks = epilogue == EPI_F32 ? gemv_dma_ksplit(K, Nw, epilogue) : 1;
            nsplit = ga.nks;
            return launch_gemv_dma(L, ga);
        };
        FL_TRY(run(B.w));
        FL_HIP(hipStreamSynchronize(B.s));
        if (iters > 0 && ms_out) {
            // the timed launches rotate over copies of W that together exceed the 256 MiB Infinity Cache: in the forward pass a
            // projection's weights always come from HBM, and a back-to-back replay on ONE copy would read them from the cache
            const size_t wbytes = (size_t)Nw * K * es;
            const int hot = tune(TK_OP_HOT);   // 1: one copy (L2 + Infinity Cache); n > 1: n copies (past the L2s, inside the Infinity Cache when n x bytes < 256 MiB)
            const int ncopy = hot > 0 ? hot : (int)std::min<size_t>(24, std::max<size_t>(1, (640u << 20) / wbytes + 1));
            std::vector<void *> &copies = B.copies;
            copies.push_back(nullptr);                                   // slot 0 = B.w itself
            for (int c = 1; c < ncopy; c++) {
                void *p = nullptr;
                FL_HIP(hipMalloc(&p, wbytes));
                copies.push_back(p);
                FL_HIP(hipMemcpyAsync(p, B.w, wbytes, hipMemcpyDeviceToDevice, B.s));
            }
            copies[0] = B.w;
            for (int c = 0; c < ncopy; c++) FL_TRY(run(copies[c]));   // warm
            FL_HIP(hipStreamSynchronize(B.s));
            FL_HIP(hipEventCreate(&B.e0)); FL_HIP(hipEventCreate(&B.e1));
            FL_HIP(hipEventRecord(B.e0, B.s));
            for (int i = 0; i < iters; i++) FL_TRY(run(copies[i % ncopy]));
            FL_HIP(hipEventRecord(B.e1, B.s));
            FL_HIP(hipEventSynchronize(B.e1));
            float ms = 0.f; FL_HIP(hipEventElapsedTime(&ms, B.e0, B.e1));
            *ms_out = ms / iters;
        }
        if (epilogue == EPI_GATEUP) {
            std::unique_ptr<unsigned char[]> tmp(new unsigned char[ybytes]);
            FL_HIP(hipMemcpy(tmp.get(), B.y, ybytes, hipMemcpyDeviceToHost));
            for (int64_t t = 0; t < T; t++)
                for (int64_t j = 0; j < I; j++) {
                    const size_t idx = (size_t)t * Ip + j;
                    y[(size_t)t * I + j] = es == 2 ? bf16_bits_to_float(reinterpret_cast<bf16_t *>(tmp.get())[idx])
                                                   : reinterpret_cast<float *>(tmp.get())[idx];
                }
        } else {
            FL_HIP(hipMemcpy(y, B.y, ybytes, hipMemcpyDeviceToHost));
            if (nsplit > 1) {                                   // sum the split-K slabs in slab order, like rmsnorm_add does
                std::unique_ptr<float[]> tmp(new float[(size_t)T * Ny]);
                for (int sl = 1; sl < nsplit; sl++) {
                    FL_HIP(hipMemcpy(tmp.get(), (char *)B.y + (size_t)sl * ybytes, ybytes, hipMemcpyDeviceToHost));
                    for (size_t i = 0; i < (size_t)T * Ny; i++) y[i] += tmp[i];
                }
            }
        }
        return FL_OK;
    });
}

int fl_op_quantize_rows(const void *w, int32_t dtype, int64_t N, int64_t K, uint8_t *q_out, float *s_out) {
    return guarded([&]() -> int {
        if (!w || !q_out || !s_out) FL_FAIL(FL_ERR_BAD_ARGUMENT, "null argument");
        if (dtype != FL_DTYPE_BF16 && dtype != FL_DTYPE_F32) FL_FAIL(FL_ERR_UNSUPPORTED, "dtype must be bf16 or f32");
        if (N <= 0 || K <= 0 || K % 4 || N > (1 << 24)) FL_FAIL(FL_ERR_BAD_ARGUMENT, "bad shape (K must be a multiple of 4)");
        int ndev = 0;
        if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) FL_FAIL(FL_ERR_NO_DEVICE, "no HIP device visible: this library has no CPU path");
        FL_HIP(hipSetDevice(0));
        struct Bufs { void *w = 0; uint8_t *q = 0; float *s = 0; hipStream_t st = 0;
                      ~Bufs() { (void)hipFree(w); (void)hipFree(q); (void)hipFree(s); if (st) (void)hipStreamDestroy(st); } } B;
        const size_t es = dtype == FL_DTYPE_BF16 ? 2 : 4;
        FL_HIP(hipStreamCreate(&B.st));
        FL_HIP(hipMalloc(&B.w, (size_t)N * K * es));
        FL_HIP(hipMalloc((void **)&B.q, (size_t)N * K));
        FL_HIP(hipMalloc((void **)&B.s, (size_t)N * 4));
        FL_HIP(hipMemcpy(B.w, w, (size_t)N * K * es, hipMemcpyHostToDevice));
        Launcher L; L.stream = B.st;
        FL_TRY(launch_quantize_rows(L, dtype, B.w, N, K, B.q, B.s, nullptr));
        FL_HIP(hipStreamSynchronize(B.st));
        FL_HIP(hipMemcpy(q_out, B.q, (size_t)N * K, hipMemcpyDeviceToHost));
        FL_HIP(hipMemcpy(s_out, B.s, (size_t)N * 4, hipMemcpyDeviceToHost));
        return FL_OK;
    });
}

int fl_op_gemv_w8(const void *x, const uint8_t *q, const float *s, const float *bias, int64_t N, int64_t K, int32_t epilogue,
                  float *y, int32_t iters, double *ms_out) {
    return guarded([&]() -> int {
        if (!x || !q || !s || !y) FL_FAIL(FL_ERR_BAD_ARGUMENT, "null argument");
        if (N <= 0 || K <= 0 || N > (1 << 24)) FL_FAIL(FL_ERR_BAD_ARGUMENT, "bad shape");
        if (epilogue != EPI_F32 && epilogue != EPI_GATEUP) FL_FAIL(FL_ERR_BAD_ARGUMENT, "epilogue must be 0 or 1");
        if (epilogue == EPI_GATEUP && ((N % 2) || bias)) FL_FAIL(FL_ERR_BAD_ARGUMENT, "gate/up needs an even row count and takes no bias");
        if (!gemv_w8_supported(N, K)) FL_FAIL(FL_ERR_UNSUPPORTED, "K must be a multiple of 16 (a lane of the FP8 stream loads 16 weights), at most 81792");
        int ndev = 0;
        if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) FL_FAIL(FL_ERR_NO_DEVICE, "no HIP device visible: this library has no CPU path");
        FL_HIP(hipSetDevice(0));
        const int64_t I = N / 2, Ip = (I + 15) / 16 * 16;
        const int64_t Nw = epilogue == EPI_GATEUP ? 2 * Ip : N;          // rows of the device matrix
        const int64_t Ny = epilogue == EPI_GATEUP ? Ip : N;
        struct Bufs { void *x = 0, *y = 0; uint8_t *q = 0, *qs = 0; float *s = 0, *ss = 0, *b = 0; hipStream_t st = 0; hipEvent_t e0 = 0, e1 = 0;
                      std::vector<uint8_t *> copies;
                      ~Bufs() { (void)hipFree(x); (void)hipFree(y); (void)hipFree(q); (void)hipFree(qs); (void)hipFree(s); (void)hipFree(ss); (void)hipFree(b);
                                for (size_t i = 1; i < copies.size(); i++) (void)hipFree(copies[i]);
                                if (st) { (void)hipStreamSynchronize(st); (void)hipStreamDestroy(st); }
                                if (e0) (void)hipEventDestroy(e0);
                                if (e1) (void)hipEventDestroy(e1); } } B;
        FL_HIP(hipStreamCreate(&B.st));
        FL_HIP(hipMalloc(&B.x, (size_t)K * 2));
        FL_HIP(hipMalloc((void **)&B.q, (size_t)Nw * K));
        FL_HIP(hipMalloc((void **)&B.s, (size_t)Nw * 4));
        const size_t ybytes = (size_t)Ny * (epilogue == EPI_GATEUP ? 2 : 4);
        FL_HIP(hipMalloc(&B.y, ybytes));
        FL_HIP(hipMemcpy(B.x, x, (size_t)K * 2, hipMemcpyHostToDevice));
        Launcher L; L.stream = B.st;
        if (epilogue == EPI_GATEUP) {
            FL_HIP(hipMalloc((void **)&B.qs, (size_t)N * K));
            FL_HIP(hipMalloc((void **)&B.ss, (size_t)N * 4));
            FL_HIP(hipMemcpy(B.qs, q, (size_t)N * K, hipMemcpyHostToDevice));
            FL_HIP(hipMemcpy(B.ss, s, (size_t)N * 4, hipMemcpyHostToDevice));
            FL_HIP(hipMemsetAsync(B.q, 0, (size_t)Nw * K, B.st));
            FL_HIP(hipMemsetAsync(B.s, 0, (size_t)Nw * 4, B.st));
            FL_TRY(launch_w8_gateup_layout(L, B.qs, B.ss, I, K, B.q, B.s));
        } else {
            FL_HIP(hipMemcpy(B.q, q, (size_t)N * K, hipMemcpyHostToDevice));
            FL_HIP(hipMemcpy(B.s, s, (size_t)N * 4, hipMemcpyHostToDevice));
            if (bias) {
                FL_HIP(hipMalloc((void **)&B.b, (size_t)N * 4));
                FL_HIP(hipMemcpy(B.b, bias, (size_t)N * 4, hipMemcpyHostToDevice));
            }
        }
        auto run = [&](const uint8_t *qp) -> int {
            GemvArgs a;
            a.W = qp; a.x = B.x; a.bias = B.b; a.out = B.y; a.N = (int)Nw; a.K = (int)K; a.epi = epilogue; a.pro = PRO_X;
            return launch_gemv_w8(L, a, B.s);
        };
        FL_TRY(run(B.q));
        FL_HIP(hipStreamSynchronize(B.st));
        if (iters > 0 && ms_out) {
            // rotate over copies of q that together exceed the 256 MiB Infinity Cache (see fl_op_linear)
            const size_t wbytes = (size_t)Nw * K;
            const int hot = tune(TK_OP_HOT);
            const int ncopy = hot > 0 ? hot : (int)std::min<size_t>(24, std::max<size_t>(1, (640u << 20) / wbytes + 1));
            B.copies.push_back(B.q);
            for (int c = 1; c < ncopy; c++) {
                uint8_t *p = nullptr;
                FL_HIP(hipMalloc((void **)&p, wbytes));
                B.copies.push_back(p);
                FL_HIP(hipMemcpyAsync(p, B.q, wbytes, hipMemcpyDeviceToDevice, B.st));
            }
            for (int c = 0; c < ncopy; c++) FL_TRY(run(B.copies[c]));   // warm
            FL_HIP(hipStreamSynchronize(B.st));
            FL_HIP(hipEventCreate(&B.e0)); FL_HIP(hipEventCreate(&B.e1));
            FL_HIP(hipEventRecord(B.e0, B.st));
            for (int i = 0; i < iters; i++) FL_TRY(run(B.copies[i % ncopy]));
            FL_HIP(hipEventRecord(B.e1, B.st));
            FL_HIP(hipEventSynchronize(B.e1));
            float ms = 0.f; FL_HIP(hipEventElapsedTime(&ms, B.e0, B.e1));
            *ms_out = ms / iters;
        }
        if (epilogue == EPI_GATEUP) {
            std::unique_ptr<bf16_t[]> tmp(new bf16_t[(size_t)Ny]);
            FL_HIP(hipMemcpy(tmp.get(), B.y, ybytes, hipMemcpyDeviceToHost));
            for (int64_t j = 0; j < I; j++) y[j] = bf16_bits_to_float(tmp[(size_t)j]);
        } else {
            FL_HIP(hipMemcpy(y, B.y, ybytes, hipMemcpyDeviceToHost));
        }
        return FL_OK;
    });
}

int fl_op_kv_copy(const void *src, void *dst, int64_t rows, int64_t width_bytes, int64_t src_pitch, int64_t dst_pitch, int32_t iters,
                  double *ms_out) {
    return guarded([&]() -> int {
        if (!src || !dst) FL_FAIL(FL_ERR_BAD_ARGUMENT, "null argument");
        if (rows < 1 || width_bytes < 2 || rows > (int64_t)1 << 31) FL_FAIL(FL_ERR_BAD_ARGUMENT, "bad shape (rows >= 1, width_bytes >= 2)");
        KvCopyJob shape;                                     // width / pitch rules: the launch's own
        shape.rows = rows; shape.width = width_bytes; shape.spitch = src_pitch; shape.dpitch = dst_pitch;
        FL_TRY(kv_copy_check(shape));
        int ndev = 0;
        if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) FL_FAIL(FL_ERR_NO_DEVICE, "no HIP device visible: this library has no CPU path");
        FL_HIP(hipSetDevice(0));
        struct Bufs { std::vector<void *> s, d; hipStream_t st = 0; hipEvent_t e0 = 0, e1 = 0;
                      ~Bufs() { if (st) (void)hipStreamSynchronize(st);
                                for (void *p : s) (void)hipFree(p);
                                for (void *p : d) (void)hipFree(p);
                                if (st) (void)hipStreamDestroy(st);
                                if (e0) (void)hipEventDestroy(e0);
                                if (e1) (void)hipEventDestroy(e1); } } B;
        const size_t sbytes = (size_t)rows * (size_t)src_pitch, dbytes = (size_t)rows * (size_t)dst_pitch;
        const bool timed = iters > 0 && ms_out;
        // timed: the launches rotate over buffer pairs that together exceed the 256 MiB Infinity Cache (see fl_op_linear)
        const int hot = tune(TK_OP_HOT);
        const int ncopy = !timed ? 1 : hot > 0 ? hot : (int)std::min<size_t>(24, std::max<size_t>(1, (640u << 20) / (sbytes + dbytes) + 1));
        FL_HIP(hipStreamCreate(&B.st));
        for (int c = 0; c < ncopy; c++) {
            void *p = nullptr;
            FL_HIP(hipMalloc(&p, sbytes)); B.s.push_back(p);
            FL_HIP(hipMemcpy(p, src, sbytes, hipMemcpyHostToDevice));
            p = nullptr;
            FL_HIP(hipMalloc(&p, dbytes)); B.d.push_back(p);
            FL_HIP(hipMemcpy(p, dst, dbytes, hipMemcpyHostToDevice));
        }
        Launcher L; L.stream = B.st;
        auto run = [&](int c) -> int {
            KvCopyJob j = shape, none;
            j.src = B.s[(size_t)c]; j.dst = B.d[(size_t)c];
            return launch_kv_copy(L, j, none);
        };
        FL_TRY(run(0));
        FL_HIP(hipStreamSynchronize(B.st));
        if (timed) {
            for (int c = 0; c < ncopy; c++) FL_TRY(run(c));   // warm
            FL_HIP(hipStreamSynchronize(B.st));
            FL_HIP(hipEventCreate(&B.e0)); FL_HIP(hipEventCreate(&B.e1));
            FL_HIP(hipEventRecord(B.e0, B.st));
            for (int i = 0; i < iters; i++) FL_TRY(run(i % ncopy));
            FL_HIP(hipEventRecord(B.e1, B.st));
            FL_HIP(hipEventSynchronize(B.e1));
            float ms = 0.f; FL_HIP(hipEventElapsedTime(&ms, B.e0, B.e1));
            *ms_out = ms / iters;
        }
        FL_HIP(hipMemcpy(dst, B.d[0], dbytes, hipMemcpyDeviceToHost));
        return FL_OK;
    });
}

int fl_op_attention(const void *q, const void *k, const void *v, int64_t T, int64_t s_past, int64_t H, int64_t Hkv, int64_t d,
                    int64_t window, int32_t kernel, int32_t nsplit, float *out) {
    return guarded([&]() -> int {
        if (!q || !k || !v || !out) FL_FAIL(FL_ERR_BAD_ARGUMENT, "null argument");
        if (T < 1 || s_past < 0 || H < 1 || Hkv < 1 || kernel < 0 || kernel > 3 || nsplit < 0 || nsplit > 64) FL_FAIL(FL_ERR_BAD_ARGUMENT, "bad shape / kernel");
        if (!attn_mfma_supported(FL_DTYPE_BF16, H, Hkv, d)) FL_FAIL(FL_ERR_UNSUPPORTED, "MFMA attention: head_dim 64 / 128, at most 8 query heads per kv head");
        if (kernel == 1 && T != 1) FL_FAIL(FL_ERR_BAD_ARGUMENT, "the decode kernel takes one query token");
        int ndev = 0;
        if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) FL_FAIL(FL_ERR_NO_DEVICE, "no HIP device visible: this library has no CPU path");
        FL_HIP(hipSetDevice(0));
        const int64_t S = s_past + T, sa = (S + 31) / 32 * 32;
        // the cache layout of the model: K [Hkv][sa][d], V transposed [Hkv][d][sa], zero padding (model.hip cache_create)
        std::vector<bf16_t> kc((size_t)Hkv * sa * d, 0), vt((size_t)Hkv * d * sa, 0);
        const bf16_t *kh = reinterpret_cast<const bf16_t *>(k), *vh = reinterpret_cast<const bf16_t *>(v);
        for (int64_t s = 0; s < S; s++)
            for (int64_t h = 0; h < Hkv; h++)
                for (int64_t j = 0; j < d; j++) {
                    kc[((size_t)h * sa + s) * d + j] = kh[((size_t)s * Hkv + h) * d + j];
                    vt[((size_t)h * d + j) * sa + s] = vh[((size_t)s * Hkv + h) * d + j];
                }
        if (nsplit == 0) nsplit = (int)std::max<int64_t>(1, std::min<int64_t>((S + 127) / 128, 48));
        struct Bufs { void *q = 0, *k = 0, *v = 0, *o = 0; StepState *st = 0; float *pm = 0, *pl = 0, *po = 0; unsigned *cnt = 0; hipStream_t s = 0;
                      ~Bufs() { (void)hipFree(q); (void)hipFree(k); (void)hipFree(v); (void)hipFree(o); (void)hipFree(st); (void)hipFree(pm);
                                (void)hipFree(pl); (void)hipFree(po); (void)hipFree(cnt); if (s) (void)hipStreamDestroy(s); } } B;
        const size_t qb = (size_t)T * H * d * 2;
        FL_HIP(hipStreamCreate(&B.s));
        FL_HIP(hipMalloc(&B.q, qb)); FL_HIP(hipMalloc(&B.o, qb));
        FL_HIP(hipMalloc(&B.k, kc.size() * 2)); FL_HIP(hipMalloc(&B.v, vt.size() * 2));
        FL_HIP(hipMalloc((void **)&B.st, sizeof(StepState)));
        FL_HIP(hipMalloc((void **)&B.pm, (size_t)H * nsplit * 4)); FL_HIP(hipMalloc((void **)&B.pl, (size_t)H * nsplit * 4));
        FL_HIP(hipMalloc((void **)&B.po, (size_t)H * nsplit * d * 4)); FL_HIP(hipMalloc((void **)&B.cnt, (size_t)H * 4));
        StepState st{}; st.pos = (uint32_t)s_past; st.len = (uint32_t)s_past; st.call0 = (uint32_t)s_past; st.eos = -1;
        FL_HIP(hipMemcpy(B.q, q, qb, hipMemcpyHostToDevice));
        FL_HIP(hipMemcpy(B.k, kc.data(), kc.size() * 2, hipMemcpyHostToDevice));
        FL_HIP(hipMemcpy(B.v, vt.data(), vt.size() * 2, hipMemcpyHostToDevice));
        FL_HIP(hipMemcpy(B.st, &st, sizeof st, hipMemcpyHostToDevice));
        FL_HIP(hipMemset(B.cnt, 0, (size_t)H * 4));
        FL_HIP(hipMemset(B.o, 0xff, qb));                         // NaN pattern: an element the kernel does not write shows up
        Launcher L; L.stream = B.s;
        const float scale = 1.0f / sqrtf((float)d);
        int rc;
        if (kernel == 1 || (kernel == 0 && T == 1)) {
            AttnScratch as{B.pm, B.pl, B.po, B.cnt, nsplit, S};
            rc = launch_attn_decode_mfma(L, B.q, B.k, B.v, B.st, B.o, as, H, Hkv, d, sa, scale);
        } else {
            attn_prefill_force(kernel);
            rc = launch_attn_prefill_mfma(L, B.q, B.k, B.v, B.st, B.o, T, H, Hkv, d, sa, scale, window < 0 ? -1 : window);
            attn_prefill_force(0);
        }
        FL_TRY(rc);
        FL_HIP(hipStreamSynchronize(B.s));
        std::vector<bf16_t> oh((size_t)T * H * d);
        FL_HIP(hipMemcpy(oh.data(), B.o, qb, hipMemcpyDeviceToHost));
        for (size_t i = 0; i < oh.size(); i++) out[i] = bf16_bits_to_float(oh[i]);
        return FL_OK;
    });
}


int fl_op_attention_plain(const void *q, const void *k, const void *v, int32_t dtype, int32_t layout, int32_t kernel, int64_t T, int64_t s_past,
                          int64_t call0, int64_t k_rows, int64_t capacity, int64_t H, int64_t Hkv, int64_t d, int64_t window, int32_t nsplit,
                          float pad_value, int32_t repeat, float *out) {
    return guarded([&]() -> int {
        if (!q || !k || !v || !out) FL_FAIL(FL_ERR_BAD_ARGUMENT, "null argument");
        if (T < 1 || s_past < 0 || call0 < 0 || call0 > s_past || kernel < 0 || kernel > 3 || (layout == 0 && kernel == 3) || nsplit < 0 || nsplit > 64 ||
            repeat < 1 || repeat > 16)
            FL_FAIL(FL_ERR_BAD_ARGUMENT, "bad shape / kernel (call0 <= s_past, nsplit 0..64, repeat 1..16; the plain layout has one prefill kernel)");
        if (kernel == 1 && T != 1) FL_FAIL(FL_ERR_BAD_ARGUMENT, "the decode kernel takes one query token");
        const int64_t S = s_past + T;
        if (k_rows < S || capacity < k_rows || capacity > (int64_t)1 << 24) FL_FAIL(FL_ERR_BAD_ARGUMENT, "s_past + T <= k_rows <= capacity");
        if (!(pad_value == pad_value) || pad_value - pad_value != 0.f) FL_FAIL(FL_ERR_BAD_ARGUMENT, "pad_value must be finite");
        FL_TRY(attn_op_check_heads(dtype, layout, H, Hkv, d));
        int ndev = 0;
        if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) FL_FAIL(FL_ERR_NO_DEVICE, "no HIP device visible: this library has no CPU path");
        FL_HIP(hipSetDevice(0));
        const bool mfma = layout == 1, decode = kernel == 1 || (kernel == 0 && T == 1);
        const int64_t sa = (capacity + 31) / 32 * 32;
        const size_t es = dtype == FL_DTYPE_BF16 ? 2 : 4, qn = (size_t)T * H * d;
        if (nsplit == 0) nsplit = attn_cache_nsplit(mfma, (size_t)capacity, d);
        AttnOpBufs B;
        FL_HIP(hipStreamCreate(&B.s));
        void *qd, *od, *kd, *vd; StepState *std_; float *pm, *pl, *po; unsigned *cnt;
        FL_TRY(B.upload(&qd, q, qn * es));
        FL_TRY(B.alloc(&od, qn * es * repeat));
        FL_HIP(hipMemset(od, 0xff, qn * es * repeat));            // NaN pattern: an element a launch does not write shows up
        FL_TRY(attn_op_upload_cache(B, &kd, &vd, dtype, k, v, 1, k_rows, Hkv, sa, d, mfma, pad_value));
        FL_TRY(attn_op_scratch(B, &pm, &pl, &po, &cnt, H, d, nsplit));
        StepState st{}; st.pos = (uint32_t)s_past; st.len = (uint32_t)s_past; st.call0 = (uint32_t)call0; st.eos = -1;
        FL_TRY(B.upload((void **)&std_, &st, sizeof st));
        Launcher L; L.stream = B.s;
        const float scale = 1.0f / sqrtf((float)d);
        const int64_t w = window < 0 ? -1 : window;
        for (int r = 0; r < repeat; r++) {                          // every launch on the same scratch and ticket words
            void *o = (char *)od + (size_t)r * qn * es;
            int rc;
            if (decode) {
                AttnScratch as{pm, pl, po, cnt, nsplit, S};
                rc = mfma ? launch_attn_decode_mfma(L, qd, kd, vd, std_, o, as, H, Hkv, d, sa, scale)
                          : launch_attn_decode(L, dtype, qd, kd, vd, std_, o, as, H, Hkv, d, sa, scale);
            } else if (mfma) {
                attn_prefill_force(kernel);
                rc = launch_attn_prefill_mfma(L, qd, kd, vd, std_, o, T, H, Hkv, d, sa, scale, w);
                attn_prefill_force(0);
            } else {
                rc = launch_attn_prefill(L, dtype, qd, kd, vd, std_, o, T, H, Hkv, d, sa, scale, w);
            }
            FL_TRY(rc);
        }
        FL_HIP(hipStreamSynchronize(B.s));
        return attn_op_download(out, od, qn * repeat, dtype);
    });
}

int fl_op_attention_batch(const void *q, const void *const *k, const void *const *v, int32_t dtype, int32_t layout, int64_t B_, const int64_t *lens,
                          const int64_t *k_rows, const int64_t *seq_alloc, const int32_t *nsplit, int64_t n_layers, int64_t layer, int64_t H,
                          int64_t Hkv, int64_t d, float pad_value, int32_t repeat, float *out) {
    return guarded([&]() -> int {
        if (!q || !k || !v || !lens || !k_rows || !seq_alloc || !nsplit || !out) FL_FAIL(FL_ERR_BAD_ARGUMENT, "null argument");
        if (B_ < 1 || B_ > 1023 || n_layers < 1 || n_layers > 64 || layer < 0 || layer >= n_layers || repeat < 1 || repeat > 16)
            FL_FAIL(FL_ERR_BAD_ARGUMENT, "bad shape (1 <= B <= 1023, layer < n_layers <= 64, repeat 1..16)");
        for (int64_t b = 0; b < B_; b++) {
            if (!k[b] || !v[b]) FL_FAIL(FL_ERR_BAD_ARGUMENT, "null argument (sequence %lld)", (long long)b);
            if (lens[b] < 1 || k_rows[b] < lens[b] || seq_alloc[b] < k_rows[b] || seq_alloc[b] % 32 != 0 || seq_alloc[b] > (int64_t)1 << 24)
                FL_FAIL(FL_ERR_BAD_ARGUMENT, "sequence %lld: 1 <= len <= k_rows <= seq_alloc, seq_alloc a multiple of 32", (long long)b);
            if (nsplit[b] < 0 || nsplit[b] > 64) FL_FAIL(FL_ERR_BAD_ARGUMENT, "sequence %lld: nsplit 0..64", (long long)b);
        }
        if (!(pad_value == pad_value) || pad_value - pad_value != 0.f) FL_FAIL(FL_ERR_BAD_ARGUMENT, "pad_value must be finite");
        FL_TRY(attn_op_check_heads(dtype, layout, H, Hkv, d));
        int ndev = 0;
        if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) FL_FAIL(FL_ERR_NO_DEVICE, "no HIP device visible: this library has no CPU path");
        FL_HIP(hipSetDevice(0));
        const bool mfma = layout == 1;
        const int nb = (int)B_;
        const size_t es = dtype == FL_DTYPE_BF16 ? 2 : 4, qn = (size_t)nb * H * d;
        AttnOpBufs B;
        FL_HIP(hipStreamCreate(&B.s));
        void *qd, *od;
        FL_TRY(B.upload(&qd, q, qn * es));
        FL_TRY(B.alloc(&od, qn * es * repeat));
        FL_HIP(hipMemset(od, 0xff, qn * es * repeat));
        // every sequence a cache of its own, as fl_batch_create finds them: K / V of all layers, step state, split scratch, ticket
        // words; the SeqRef fields the attention kernels do not read stay null
        std::vector<SeqRef> refs((size_t)nb);
        int max_nsplit = 1;
        for (int b = 0; b < nb; b++) {
            SeqRef &r = refs[(size_t)b];
            r = SeqRef{};
            r.seq_alloc = (int)seq_alloc[b];
            r.nsplit = nsplit[b] > 0 ? nsplit[b] : attn_cache_nsplit(mfma, (size_t)seq_alloc[b], d);
            max_nsplit = std::max(max_nsplit, r.nsplit);
            FL_TRY(attn_op_upload_cache(B, &r.k, &r.v, dtype, k[b], v[b], n_layers, k_rows[b], Hkv, seq_alloc[b], d, mfma, pad_value));
            FL_TRY(attn_op_scratch(B, &r.part_m, &r.part_l, &r.part_o, &r.counters, H, d, r.nsplit));
            StepState st{}; st.pos = (uint32_t)(lens[b] - 1); st.len = (uint32_t)(lens[b] - 1); st.call0 = st.len; st.eos = -1;
            FL_TRY(B.upload((void **)&r.st, &st, sizeof st));
        }
        SeqRef *seqs_dev;
        FL_TRY(B.upload((void **)&seqs_dev, refs.data(), sizeof(SeqRef) * (size_t)nb));
        Launcher L; L.stream = B.s;
        const float scale = 1.0f / sqrtf((float)d);
        const size_t kv_layer_off = (size_t)(layer * Hkv * d);
        for (int r = 0; r < repeat; r++) {
            void *o = (char *)od + (size_t)r * qn * es;
            if (mfma) FL_TRY(launch_attn_decode_mfma_batch(L, qd, seqs_dev, nb, max_nsplit, kv_layer_off, o, H, Hkv, d, scale, 0.0));
            else FL_TRY(launch_attn_decode_batch(L, dtype, qd, seqs_dev, nb, max_nsplit, kv_layer_off, o, H, Hkv, d, scale));
        }
        FL_HIP(hipStreamSynchronize(B.s));
        return attn_op_download(out, od, qn * repeat, dtype);
    });
}

}  // extern "C"
