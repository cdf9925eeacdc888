// k_ops.hip -- the small memory-bound ops of the decoder: embedding gather (K1), fused
// residual-add + RMSNorm (K2/K9), RoPE + KV-cache append (K4/K5), device argmax (K13),
// local shard reduction, and the one-off weight conversion at model build.
#include <stdlib.h>

#include "kernels.h"
#include "sampler_dev.h"     // the seeded stream, the ordered sums, top_filter and sample_all (shared with k_verify_sample.hip)
#include "argmax_dev.h"      // one row's ArgMax by one workgroup (shared with k_verify_packed.hip)
#include "logprobs_dev.h"    // the two passes over a row behind a reported log-prob (shared with k_score.hip)

namespace fl {

static const char *kNames[KC_COUNT] = {
    "embed", "rmsnorm_add", "gemv", "gemm_mfma", "gemm_generic", "rope_kv_append", "attn_decode",
    "attn_combine", "attn_prefill", "select_advance", "reduce_shards", "convert", "attn_oproj", "comm_oneshot", "kv_copy",
    "encoder_embed_ln", "encoder_add_ln", "encoder_bias_gelu", "encoder_attention", "encoder_pool_l2"};
const char *kernel_class_name(int kc) { return (kc >= 0 && kc < KC_COUNT) ? kNames[kc] : "?"; }

// ------------------------------------------------------------------------------- embedding
// Embedding::forward (index_select): x[t,:] = E[ids[t],:]; residual stream is fp32.
template <typename WT>
__global__ __launch_bounds__(256) void embed_kernel(const WT *__restrict__ E, const uint32_t *__restrict__ ids,
                                                    const StepState *__restrict__ st, float *__restrict__ x, int h) {
    const int t = blockIdx.x;
    const uint32_t id = ids ? ids[t] : st->token;
    const WT *row = E + (size_t)id * h;
    float *dst = x + (size_t)t * h;
    for (int c = threadIdx.x; c * 8 < h; c += 256) {
        float v[8];
        load8(row + c * 8, v);
        store8(dst + c * 8, v);
    }
}

int launch_embed(Launcher &L, int dtype, const void *E, const uint32_t *ids, const StepState *st,
                 float *x_res, int64_t T, int64_t h) {
    double bytes = (double)T * h * ((dtype == FL_DTYPE_BF16 ? 2 : 4) + 4);
    if (dtype == FL_DTYPE_BF16)
        return L.launch(KC_EMBED, bytes, 0, embed_kernel<bf16_t>, dim3((unsigned)T), dim3(256), 0,
                        (const bf16_t *)E, ids, st, x_res, (int)h);
    return L.launch(KC_EMBED, bytes, 0, embed_kernel<float>, dim3((unsigned)T), dim3(256), 0,
                    (const float *)E, ids, st, x_res, (int)h);
}

// ------------------------------------------------------------------------------- rmsnorm (+add)
// candle_nn::ops::rms_norm (App. A.2): m = sqrt(sum(x^2)/h + eps), y = x / m * w, sum in fp32.
// Fused with the preceding residual add (x_res += delta) so the residual stream is read once.
// Emits xs = x * w and inv_rms = 1/m separately: y = inv_rms * xs is finished by the consumer's
// epilogue (single pass over x here, and the same rounding point as the fused decode prologue).
template <typename OT>
__global__ __launch_bounds__(256) void rmsnorm_add_kernel(float *__restrict__ x_res, const float *__restrict__ delta,
                                                          const float *__restrict__ w, float eps,
                                                          OT *__restrict__ xs, float *__restrict__ inv_rms, int h,
                                                          int n_slab, long long slab_stride) {
    __shared__ float red[4];
    const int t = blockIdx.x, tid = threadIdx.x;
    float *xr = x_res + (size_t)t * h;
    const float *dr = delta ? delta + (size_t)t * h : nullptr;
    float ss = 0.f;
    for (int c = tid; c * 8 < h; c += 256) {
        float v[8], wv[8], o[8];
        load8(xr + c * 8, v);
        load8(w + c * 8, wv);
        if (dr) {
            // split-K slabs, summed in slab order; four are requested at a time (one slab per round trip made this launch a
            // latency chain at eight slabs: Mistral-7B T = 512 13.3 us)
            for (int sl = 0; sl < n_slab; sl += 4) {
                float d[4][8];
#pragma unroll
                for (int u = 0; u < 4; u++)
                    if (sl + u < n_slab) load8(dr + (size_t)(sl + u) * slab_stride + c * 8, d[u]);
#pragma unroll
                for (int u = 0; u < 4; u++)
                    if (sl + u < n_slab) {
#pragma unroll
                        for (int j = 0; j < 8; j++) v[j] += d[u][j];
                    }
            }
            store8(xr + c * 8, v);
        }
#pragma unroll
        for (int j = 0; j < 8; j++) { ss = fmaf(v[j], v[j], ss); o[j] = v[j] * wv[j]; }
        store8(xs + (size_t)t * h + c * 8, o);
    }
    ss = wave_sum(ss);
    if ((tid & 63) == 0) red[tid >> 6] = ss;
    __syncthreads();
    if (tid == 0) inv_rms[t] = 1.0f / sqrtf((red[0] + red[1] + red[2] + red[3]) / (float)h + eps);
}

int launch_rmsnorm_add(Launcher &L, int dtype, float *x_res, const float *delta, const float *w, float eps,
                       void *xs, float *inv_rms, int64_t T, int64_t h, int n_slab, int64_t slab_stride) {
    double bytes = (double)T * h * (4.0 * (delta ? 2 + n_slab : 1) + (dtype == FL_DTYPE_BF16 ? 2 : 4));
    if (dtype == FL_DTYPE_BF16)
        return L.launch(KC_RMSNORM, bytes, 0, rmsnorm_add_kernel<bf16_t>, dim3((unsigned)T), dim3(256), 0,
                        x_res, delta, w, eps, (bf16_t *)xs, inv_rms, (int)h, n_slab, (long long)slab_stride);
    return L.launch(KC_RMSNORM, bytes, 0, rmsnorm_add_kernel<float>, dim3((unsigned)T), dim3(256), 0,
                    x_res, delta, w, eps, (float *)xs, inv_rms, (int)h, n_slab, (long long)slab_stride);
}

// 1/rms from the partial sums of squares the EPI_RESID GEMM epilogue left (kernels.h): one wave per row, fixed tree order
__global__ __launch_bounds__(256) void rms_finalize_kernel(const float *__restrict__ part, int np, float eps, float *__restrict__ inv_rms, int T, int h) {
    const int t = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (t >= T) return;
    float ss = 0.f;
    for (int i = lane; i < np; i += 64) ss += part[(size_t)t * np + i];
    ss = wave_sum(ss);
    if (lane == 0) inv_rms[t] = 1.0f / sqrtf(ss / (float)h + eps);
}
int rs_parts_to_vector(Launcher &L, const float *row_scale, int64_t T) {
    if (!L.rsp.part) return FL_OK;
    if (!row_scale || !(L.rsp.inv_h > 0.f)) FL_FAIL(FL_ERR_BAD_ARGUMENT, "row scales left as partial sums, and no vector to finish them into");
    const RsParts p = L.rsp;
    L.rsp = RsParts{};
    return launch_rms_finalize(L, p.part, p.np, p.eps, const_cast<float *>(row_scale), T, (int64_t)(1.0f / p.inv_h + 0.5f));
}

int launch_rms_finalize(Launcher &L, const float *part, int np, float eps, float *inv_rms, int64_t T, int64_t h) {
    Launcher LL = L; LL.tag = "finalize";
    return LL.launch(KC_RMSNORM, (double)T * np * 4.0, 0, rms_finalize_kernel, dim3((unsigned)((T + 3) / 4)), dim3(256), 0, part, np, eps, inv_rms,
                     (int)T, (int)h);
}

// ------------------------------------------------------------------------------- RoPE + KV append
// candle_nn::rotary_emb::rope (rotate-half, App. A.4) on q and k, then the new K/V rows are
// written in place at cache index len+t (the reference's Tensor::cat copies the whole cache every
// step, K5).  One thread per (t, head, j < d/2) pair.  cos/sin come from host-built fp32 tables.
// The arithmetic is rope_kv_load / rope_kv_store (common.h), shared with the batched and the packed form: a kernel resolves its row.
template <typename CT>
__global__ __launch_bounds__(256) void rope_kv_kernel(const float *__restrict__ qkv, const StepState *__restrict__ st,
                                                      const float *__restrict__ cos_tab, const float *__restrict__ sin_tab,
                                                      int max_pos, CT *__restrict__ q_out, CT *__restrict__ kc,
                                                      CT *__restrict__ vc, int T, int H, int Hkv, int d, int max_seq,
                                                      int v_transposed, int nslab, const float *__restrict__ bias) {
    RopeKvPair p;
    if (!rope_kv_load(qkv, (long long)blockIdx.x * 256 + threadIdx.x, T, H, Hkv, d, nslab, bias, p)) return;
    void *const k = kc, *const v = vc;
    const RopeKvDst dst{q_out + (size_t)p.r * H * d, &k, &v, 0, (size_t)max_seq, &v_transposed};
    rope_kv_store<CT>(p, st->pos + (uint32_t)p.r, st->len + (uint32_t)p.r, cos_tab, sin_tab, max_pos, H, Hkv, d, dst);
}

// The prompt-sized form (bf16, transposed value cache, T > 1): 8 pairs per thread with 16-byte loads / stores for q and k,
// and V through a 32-token x 64-row LDS transpose so that the value cache [Hkv][d][seq] receives 64-byte runs of
// consecutive tokens instead of one strided 2-byte store per element (Mistral-7B T = 512: 11 -> ~6 us per layer).
// Blocks [0, nA): 256 (token, q-or-k head, 8-pair chunk) items each; blocks [nA, ..): one V tile each.
__global__ __launch_bounds__(256) void rope_kv_vec_kernel(const float *__restrict__ qkv, const StepState *__restrict__ st,
                                                          const float *__restrict__ cos_tab, const float *__restrict__ sin_tab,
                                                          int max_pos, bf16_t *__restrict__ q_out, bf16_t *__restrict__ kc,
                                                          bf16_t *__restrict__ vc, int T, int H, int Hkv, int d, int max_seq,
                                                          int nslab, long long slab_stride, int nA, const float *__restrict__ bias) {
    __shared__ bf16_t tile[64][40];                       // [d row][token], 80-byte rows: 16-byte aligned chunks of 8 tokens
    const int half = d >> 1, nheads = H + 2 * Hkv, tid = threadIdx.x;
    const uint32_t len = st->len, pos0 = st->pos;
    if ((int)blockIdx.x < nA) {
        const int cph = half >> 3;                        // 8-pair chunks per head
        const long long idx = (long long)blockIdx.x * 256 + tid;
        if (idx >= (long long)T * (H + Hkv) * cph) return;
        const int t = (int)(idx / ((H + Hkv) * cph)), rem = (int)(idx % ((H + Hkv) * cph));
        const int hd = rem / cph, j0 = (rem % cph) * 8;
        const float *src = qkv + (size_t)t * nheads * d + (size_t)hd * d + j0;
        float a[8], b[8];
        load8(src, a); load8(src + half, b);
        for (int sl = 1; sl < nslab; sl++) {              // split-K slabs of the projection, summed in slab order
            float a2[8], b2[8];
            load8(src + (size_t)sl * slab_stride, a2); load8(src + (size_t)sl * slab_stride + half, b2);
#pragma unroll
            for (int j = 0; j < 8; j++) { a[j] += a2[j]; b[j] += b2[j]; }
        }
        if (bias) {
            float ba[8], bb[8];
            load8(bias + (size_t)hd * d + j0, ba); load8(bias + (size_t)hd * d + j0 + half, bb);
#pragma unroll
            for (int j = 0; j < 8; j++) { a[j] += ba[j]; b[j] += bb[j]; }
        }
        const uint32_t pos = pos0 + (uint32_t)t, p = pos < (uint32_t)max_pos ? pos : (uint32_t)max_pos - 1;
        float c[8], sn[8], ra[8], rb[8];
        load8(cos_tab + (size_t)p * half + j0, c); load8(sin_tab + (size_t)p * half + j0, sn);
#pragma unroll
        for (int j = 0; j < 8; j++) rope_rotate_exact(a[j], b[j], c[j], sn[j], ra[j], rb[j]);     // (separately rounded products, as the scalar kernels)
        bf16_t *o = hd < H ? q_out + ((size_t)t * H + hd) * d + j0 : kc + ((size_t)(hd - H) * max_seq + len + t) * d + j0;
        store8(o, ra); store8(o + half, rb);
        return;
    }
    // ---- V tile: 32 tokens x 64 d rows of one kv head ----
    const int vb = (int)blockIdx.x - nA, dpt = d / 64;    // d tiles per head
    const int tt = vb / (Hkv * dpt), hk = (vb / dpt) % Hkv, d0 = (vb % dpt) * 64, t0 = tt * 32;
    {
        const int tl = tid >> 3, t = t0 + tl, j0 = (tid & 7) * 8;
        if (t < T) {
            const float *src = qkv + (size_t)t * nheads * d + (size_t)(H + Hkv + hk) * d + d0 + j0;
            float v[8];
            load8(src, v);
            for (int sl = 1; sl < nslab; sl++) {
                float v2[8];
                load8(src + (size_t)sl * slab_stride, v2);
#pragma unroll
                for (int j = 0; j < 8; j++) v[j] += v2[j];
            }
            if (bias) {
                float bv[8];
                load8(bias + (size_t)(H + Hkv + hk) * d + d0 + j0, bv);
#pragma unroll
                for (int j = 0; j < 8; j++) v[j] += bv[j];
            }
#pragma unroll
            for (int j = 0; j < 8; j++) tile[j0 + j][tl] = float_to_bf16_bits(v[j]);
        }
    }
    __syncthreads();
    const int r = tid >> 2, c8 = (tid & 3) * 8;           // d row, first of 8 tokens
    bf16_t *dst = vc + ((size_t)hk * d + d0 + r) * max_seq + len + t0 + c8;
    if (t0 + c8 + 8 <= T && ((len + t0 + c8) & 7) == 0) {
        *reinterpret_cast<uint4v *>(dst) = *reinterpret_cast<const uint4v *>(&tile[r][c8]);
    } else {
        for (int j = 0; j < 8 && t0 + c8 + j < T; j++) dst[j] = tile[r][c8 + j];
    }
}

bool rope_kv_takes_vec(int dtype, bool v_transposed, int64_t T, int64_t d, int64_t max_seq) {
    return tune(TK_ROPE_VEC) && dtype == FL_DTYPE_BF16 && v_transposed && T >= 16 && d % 64 == 0 && max_seq % 8 == 0;
}

int launch_rope_kv(Launcher &L, int dtype, const float *qkv, const StepState *st, const float *cos_tab,
                   const float *sin_tab, int64_t max_pos, void *q_out, void *k_cache, void *v_cache,
                   int64_t T, int64_t H, int64_t Hkv, int64_t d, int64_t max_seq, bool v_transposed, int nslab, const float *bias) {
    const long long slab_stride = (long long)T * (H + 2 * Hkv) * d;
    const int64_t total = T * (H + 2 * Hkv) * (d / 2);
    const unsigned blocks = (unsigned)((total + 255) / 256);
    const int es = dtype == FL_DTYPE_BF16 ? 2 : 4;
    double bytes = (double)T * (H + 2 * Hkv) * d * (4 + es);
    if (rope_kv_takes_vec(dtype, v_transposed, T, d, max_seq)) {
        const int64_t itemsA = T * (H + Hkv) * (d / 16);
        const int nA = (int)((itemsA + 255) / 256), nB = (int)(((T + 31) / 32) * Hkv * (d / 64));
        return L.launch(KC_ROPE_KV, bytes, 0, rope_kv_vec_kernel, dim3((unsigned)(nA + nB)), dim3(256), 0, qkv, st, cos_tab, sin_tab,
                        (int)max_pos, (bf16_t *)q_out, (bf16_t *)k_cache, (bf16_t *)v_cache, (int)T, (int)H, (int)Hkv, (int)d,
                        (int)max_seq, nslab, slab_stride, nA, bias);
    }
    if (dtype == FL_DTYPE_BF16)
        return L.launch(KC_ROPE_KV, bytes, 0, rope_kv_kernel<bf16_t>, dim3(blocks), dim3(256), 0, qkv, st, cos_tab,
                        sin_tab, (int)max_pos, (bf16_t *)q_out, (bf16_t *)k_cache, (bf16_t *)v_cache, (int)T, (int)H,
                        (int)Hkv, (int)d, (int)max_seq, (int)v_transposed, nslab, bias);
    return L.launch(KC_ROPE_KV, bytes, 0, rope_kv_kernel<float>, dim3(blocks), dim3(256), 0, qkv, st, cos_tab,
                    sin_tab, (int)max_pos, (float *)q_out, (float *)k_cache, (float *)v_cache, (int)T, (int)H,
                    (int)Hkv, (int)d, (int)max_seq, (int)v_transposed, nslab, bias);
}

// ------------------------------------------------------------------------------- batched variants (row N4)
// One row per sequence of a batch: the token, RoPE position, KV slot and caches come from its SeqRef.
template <typename WT>
__global__ __launch_bounds__(256) void embed_batch_kernel(const WT *__restrict__ E, const SeqRef *__restrict__ seqs,
                                                          float *__restrict__ x, int h) {
    const int b = blockIdx.x;
    const WT *row = E + (size_t)seqs[b].st->token * h;
    float *dst = x + (size_t)b * h;
    for (int c = threadIdx.x; c * 8 < h; c += 256) {
        float v[8];
        load8(row + c * 8, v);
        store8(dst + c * 8, v);
    }
}

int launch_embed_batch(Launcher &L, const void *E, const SeqRef *seqs_dev, float *x_res, int B, int64_t h, int dtype) {
    if (dtype == FL_DTYPE_F32)
        return L.launch(KC_EMBED, (double)B * h * 8, 0, embed_batch_kernel<float>, dim3((unsigned)B), dim3(256), 0, (const float *)E, seqs_dev, x_res, (int)h);
    return L.launch(KC_EMBED, (double)B * h * 6, 0, embed_batch_kernel<bf16_t>, dim3((unsigned)B), dim3(256), 0, (const bf16_t *)E, seqs_dev,
                    x_res, (int)h);
}

// qkv fp32 [B][(H+2Hkv)*d] -> RoPE -> q bf16 [B][H*d], rotated k and v appended to each sequence's own cache
// (V transposed, the MFMA attention layout); kv_layer_off = layer * Hkv * d, times the sequence's seq_alloc
template <typename CT, bool VT>
__global__ __launch_bounds__(256) void rope_kv_batch_kernel(const float *__restrict__ qkv, const SeqRef *__restrict__ seqs,
                                                            const float *__restrict__ cos_tab, const float *__restrict__ sin_tab,
                                                            int max_pos, CT *__restrict__ q_out, size_t kv_layer_off, int B,
                                                            int H, int Hkv, int d, int n_slab, const float *__restrict__ bias) {
    RopeKvPair p;
    if (!rope_kv_load(qkv, (long long)blockIdx.x * 256 + threadIdx.x, B, H, Hkv, d, n_slab, bias, p)) return;
    const SeqRef &sq = seqs[p.r];
    const size_t sa = (size_t)sq.seq_alloc;
    const int vt = VT;
    const RopeKvDst dst{q_out + (size_t)p.r * H * d, &sq.k, &sq.v, kv_layer_off * sa, sa, &vt};
    rope_kv_store<CT>(p, sq.st->pos, sq.st->len, cos_tab, sin_tab, max_pos, H, Hkv, d, dst);
}

int launch_rope_kv_batch(Launcher &L, const float *qkv, const SeqRef *seqs_dev, const float *cos_tab, const float *sin_tab,
                         int64_t max_pos, void *q_out, size_t kv_layer_off, int B, int64_t H, int64_t Hkv, int64_t d, int n_slab,
                         const float *bias, int dtype, bool v_transposed) {
    const int64_t total = (int64_t)B * (H + 2 * Hkv) * (d / 2);
    const dim3 grid((unsigned)((total + 255) / 256));
    const double bytes = (double)B * (H + 2 * Hkv) * d * (dtype == FL_DTYPE_F32 ? 8 : 6);
    if (dtype == FL_DTYPE_F32)
        return L.launch(KC_ROPE_KV, bytes, 0, rope_kv_batch_kernel<float, false>, grid, dim3(256), 0, qkv, seqs_dev, cos_tab, sin_tab, (int)max_pos,
                        (float *)q_out, kv_layer_off, B, (int)H, (int)Hkv, (int)d, n_slab, bias);
    if (!v_transposed)
        return L.launch(KC_ROPE_KV, bytes, 0, rope_kv_batch_kernel<bf16_t, false>, grid, dim3(256), 0, qkv, seqs_dev, cos_tab, sin_tab, (int)max_pos,
                        (bf16_t *)q_out, kv_layer_off, B, (int)H, (int)Hkv, (int)d, n_slab, bias);
    return L.launch(KC_ROPE_KV, bytes, 0, rope_kv_batch_kernel<bf16_t, true>, grid, dim3(256), 0, qkv, seqs_dev, cos_tab, sin_tab, (int)max_pos,
                    (bf16_t *)q_out, kv_layer_off, B, (int)H, (int)Hkv, (int)d, n_slab, bias);
}

// ------------------------------------------------------------------------------- token selection + advance
// LogitsProcessor::sample (mod.rs:308-310,425-428) on the device, then the loop-carried state of
// mod.rs:411-453 (token, pos, len, step, eos) is advanced so that a captured decode graph can be
// replayed back to back with no host round trip.
//
// argmax_reduce / argmax_last: argmax_dev.h (shared with k_verify_packed.hip)

// ArgMax over the candidates the lm_head launch left (GemvArgs::amax: one per workgroup, ties -> the larger index):
// the same result as argmax_last over the logits they were taken from, without reading the vocabulary again
__device__ inline int argmax_candidates(const ArgmaxCand *__restrict__ cand, float *bv, int *bi) {
    const int n = cand[0].i, tid = threadIdx.x;
    float best = -INFINITY; int idx = -1;
    if (tid < n) { const ArgmaxCand c = cand[1 + tid]; best = c.v; idx = c.i; }
    return argmax_reduce(best, idx, bv, bi);
}

__device__ __forceinline__ void select_advance_body(const float *__restrict__ logits, int V, StepState *__restrict__ st,
                                           SampleState *__restrict__ ss, float *__restrict__ scratch,
                                           uint32_t *__restrict__ out_tokens, int advance, unsigned char *lds,
                                           const ArgmaxCand *__restrict__ cand = nullptr) {
    __shared__ float bv[16], bcast[2];
    __shared__ int bi[16], count;
    const int tid = threadIdx.x;
    int idx;
    if (ss->on) idx = sample_all(logits, V, ss, scratch, bv, lds, bcast, &count);
    else if (cand) idx = argmax_candidates(cand, bv, bi);
    else idx = argmax_last(logits, V, bv, bi);
    if (tid == 0) {
        const uint32_t tok = (uint32_t)idx;
        if (out_tokens) out_tokens[st->step] = tok;
        st->token = tok;
        if (st->eos >= 0 && tok == (uint32_t)st->eos) st->done = 1;
        if (advance) { st->pos += 1; st->len += 1; st->step += 1; }
    }
}

__global__ __launch_bounds__(1024) void select_advance_kernel(const float *__restrict__ logits, int V,
                                                              StepState *__restrict__ st, SampleState *__restrict__ ss,
                                                              float *__restrict__ scratch, uint32_t *__restrict__ out_tokens,
                                                              int advance, const ArgmaxCand *__restrict__ cand, uint32_t *epoch_bump) {
    __shared__ __attribute__((aligned(16))) unsigned char lds[kSelLds];
    // the persistent decode engine's tag epoch (k_engine.hip): one step per forward, so no two launches ever share a tag
    if (epoch_bump && threadIdx.x == 0) *epoch_bump += 1;
    select_advance_body(logits, V, st, ss, scratch, out_tokens, advance, lds, cand);
}

// one workgroup per sequence of a batch: logits [B][V], state and scratch from the SeqRef
__global__ __launch_bounds__(1024) void select_advance_batch_kernel(const float *__restrict__ logits, int V,
                                                                    const SeqRef *__restrict__ seqs, int advance) {
    __shared__ __attribute__((aligned(16))) unsigned char lds[kSelLds];
    const SeqRef sq = seqs[blockIdx.x];
    select_advance_body(logits + (size_t)blockIdx.x * V, V, sq.st, sq.ss, sq.sel_scratch, sq.out_tokens, advance, lds);
}

int launch_select_advance_batch(Launcher &L, const float *logits, int64_t V, const SeqRef *seqs_dev, int B, int advance) {
    return L.launch(KC_ARGMAX, (double)V * 4 * B, 0, select_advance_batch_kernel, dim3((unsigned)B), dim3(1024), 0, logits, (int)V,
                    seqs_dev, advance);
}

// a tensor-parallel batch's gathered logits [tp][B][Vs] (rank-major: what one all-gather of every rank's [B][Vs] block leaves) ->
// [B][V] (V = tp * Vs), the layout token selection and fl_batch_forward's caller read
__global__ __launch_bounds__(256) void unshard_logits_kernel(const float *__restrict__ in, float *__restrict__ out, int tp, int B, int Vs) {
    const long long i = ((long long)blockIdx.x * 256 + threadIdx.x) * 4, n = (long long)tp * B * Vs;
    if (i >= n) return;
    const int r = (int)(i / ((long long)B * Vs)), rem = (int)(i % ((long long)B * Vs)), b = rem / Vs, j = rem % Vs;     // (Vs % 4 == 0: a float4 stays in its row)
    *reinterpret_cast<float4v *>(out + ((size_t)b * tp + r) * Vs + j) = *reinterpret_cast<const float4v *>(in + i);
}
int launch_unshard_logits(Launcher &L, const float *in, float *out, int tp, int B, int64_t Vs) {
    if (Vs % 4) FL_FAIL(FL_ERR_UNSUPPORTED, "a tensor-parallel batch needs a vocabulary shard that is a multiple of 4");
    const long long n = (long long)tp * B * Vs;
    return L.launch(KC_ARGMAX, (double)n * 8, 0, unshard_logits_kernel, dim3((unsigned)((n / 4 + 255) / 256)), dim3(256), 0, in, out, tp, B, (int)Vs);
}

// scratch: V floats (probabilities / cumulative weights of the sampling path)
int launch_select_advance(Launcher &L, const float *logits, int64_t V, StepState *st, SampleState *ss, float *scratch,
                          uint32_t *out_tokens, int advance, const ArgmaxCand *cand, uint32_t *epoch_bump) {
    return L.launch(KC_ARGMAX, (double)V * 4, 0, select_advance_kernel, dim3(1), dim3(1024), 0, logits, (int)V, st, ss,
                    scratch, out_tokens, advance, cand, epoch_bump);
}

// ------------------------------------------------------------------------------- verify step: ArgMax per row + acceptance scan
// fl_forward_verify: logits [T][V] of the ids [token, draft[0..T-1)].  One workgroup of 1024 lanes per row takes its row's ArgMax
// with argmax_last (ties -> the last maximal index, NaN as in select_advance) and publishes it; the workgroup that arrives last
// (one atomic ticket; nobody waits for anybody) scans the at most 16 ids: n_acc = the largest j <= T - 1 with draft[i] == a[i] for
// all i < j.  out: [0, T) the ArgMax ids, [kVerifyNacc] n_acc, [kVerifyTicket] the ticket, which the last workgroup puts back to 0
// so that the launch can be repeated (or captured) without a memset.
// (One workgroup per row, not a candidate pass over several: at V = 152 064 a row is 608 KB, which 1024 lanes fetch in five round
// trips of eight 16-byte loads -- the 16 rows run on 16 CUs side by side and the launch is a few microseconds next to a forward of
// milliseconds.)
__global__ __launch_bounds__(1024) void verify_select_kernel(const float *__restrict__ logits, int V, int T,
                                                             const uint32_t *__restrict__ draft, uint32_t *__restrict__ out) {
    __shared__ float bv[16];
    __shared__ int bi[16];
    const int row = blockIdx.x;
    const int idx = argmax_last(logits + (size_t)row * V, V, bv, bi);
    if (threadIdx.x != 0) return;
    __hip_atomic_store(&out[row], (uint32_t)idx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __threadfence();                                                   // the id is visible before the ticket is
    const uint32_t ticket = __hip_atomic_fetch_add(&out[kVerifyTicket], 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
    if (ticket != (uint32_t)(T - 1)) return;
    __threadfence();
    uint32_t n = 0;
    while (n < (uint32_t)(T - 1) && draft[n] == __hip_atomic_load(&out[n], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) n++;
    out[kVerifyNacc] = n;
    __hip_atomic_store(&out[kVerifyTicket], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

int launch_verify_select(Launcher &L, const float *logits, int64_t V, int T, const uint32_t *draft, uint32_t *out) {
    if (T < 1 || T > kVerifyMaxRows || V <= 0 || V > 0x7fffffff) FL_FAIL(FL_ERR_BAD_ARGUMENT, "verify_select: bad shape");
    return L.launch(KC_ARGMAX, (double)V * 4 * T, 0, verify_select_kernel, dim3((unsigned)T), dim3(1024), 0, logits, (int)V, T, draft, out);
}

// ------------------------------------------------------------------------------- token log-probabilities (fl_*_lp)
// The row token selection just drew from, scored by the two passes of logprobs_dev.h (shared with score_rows_kernel, k_score.hip): a
// launch of its own right behind select_advance.
__global__ __launch_bounds__(1024) void token_logprobs_kernel(const float *__restrict__ logits, int V, LogprobSrc src, int advance) {
    __shared__ __attribute__((aligned(16))) LogprobLds S;
    const int row = blockIdx.x;
    const LogprobCtl *ctl;
    uint32_t tok, slot;
    if (src.chosen) { ctl = src.ctl; tok = src.chosen[row]; slot = (uint32_t)row; }
    else {
        const StepState *st = src.seqs ? src.seqs[row].st : src.st;
        ctl = src.ctls ? src.ctls[row] : src.ctl;
        tok = st->token; slot = st->step - (uint32_t)advance;          // select_advance has advanced step already when advance is 1
    }
    if (slot >= ctl->cap) return;                                        // (workgroup-uniform; also step < advance)
    LogprobRec *__restrict__ rec = ctl->recs + slot;
    const int top_n = max(0, min(min(ctl->top_n, kLogprobsMaxTop), V));
    logprobs_row<false>(S, logits + (size_t)row * V, V, top_n, tok, &rec->chosen, rec->ids, rec->lps, nullptr);
}

int launch_token_logprobs(Launcher &L, const float *logits, int64_t V, int rows, const LogprobSrc &src, int advance) {
    if (rows < 1 || V <= 0 || V > 0x7fffffff) FL_FAIL(FL_ERR_BAD_ARGUMENT, "token_logprobs: bad shape");
    const char *tag = L.tag;
    L.tag = "logprobs";                                                  // (the profile lists it apart from the selection launch)
    const int rc = L.launch(KC_ARGMAX, (double)V * 8 * rows, 0, token_logprobs_kernel, dim3((unsigned)rows), dim3(1024), 0, logits, (int)V, src, advance);
    L.tag = tag;
    return rc;
}

__global__ void set_logprob_ctl_kernel(LogprobCtl *ctl, LogprobRec *recs, uint32_t cap, int top_n) {
    if (threadIdx.x == 0) { ctl->recs = recs; ctl->cap = cap; ctl->top_n = top_n; }
}
int launch_set_logprob_ctl(Launcher &L, LogprobCtl *ctl, LogprobRec *recs, uint32_t cap, int top_n) {
    const char *tag = L.tag;
    L.tag = "logprobs";
    const int rc = L.launch(KC_ARGMAX, 0, 0, set_logprob_ctl_kernel, dim3(1), dim3(64), 0, ctl, recs, cap, top_n);
    L.tag = tag;
    return rc;
}

// ------------------------------------------------------------------------------- local shard reduce
// FL_TP_EMULATED: all shards live on one GPU, so all-reduce(sum) is a local sum written back to
// every shard's buffer.  Fixed summation order s = 0..n-1 (reproducible).
__global__ __launch_bounds__(256) void reduce_shards_kernel(float *const *__restrict__ bufs, int nshards, long long n) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float s = 0.f;
    for (int k = 0; k < nshards; k++) s += bufs[k][i];
    for (int k = 0; k < nshards; k++) bufs[k][i] = s;
}

int launch_reduce_shards(Launcher &L, float *const *bufs_dev, int nshards, int64_t n) {
    return L.launch(KC_REDUCE, (double)n * 8 * nshards, 0, reduce_shards_kernel, dim3((unsigned)((n + 255) / 256)),
                    dim3(256), 0, bufs_dev, nshards, (long long)n);
}

// ------------------------------------------------------------------------------- weight conversion
__device__ inline float load_as_f32(const void *p, size_t i, int dt) {
    if (dt == FL_DTYPE_F32) return reinterpret_cast<const float *>(p)[i];
    if (dt == FL_DTYPE_BF16) return bf16_bits_to_float(reinterpret_cast<const bf16_t *>(p)[i]);
    return (float)reinterpret_cast<const _Float16 *>(p)[i];
}

template <typename DT>
__global__ __launch_bounds__(256) void convert_slice_kernel(const void *__restrict__ src, int src_dt, long long src_ld,
                                                            long long r0, long long c0, long long rows, long long cols,
                                                            DT *__restrict__ dst, long long dst_ld, long long dst_row0,
                                                            int row_mode, int head_pad, int dm, int d, int via_bf16) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= rows * cols) return;
    const long long r = i / cols, c = i % cols;
    float v = load_as_f32(src, (size_t)((r0 + r) * src_ld + c0 + c), src_dt);
    if (via_bf16) v = bf16_bits_to_float(float_to_bf16_bits(v));
    long long dr = row_mode == 0 ? dst_row0 + r : gateup_row(r, row_mode == 2), dc = c;
    // head_pad: element j of a head of the model's head_dim dm goes to j (first half) or d/2 + j - dm/2 (second half) of a padded
    // head of d: rotate-half partners stay d/2 apart; 1 = the slice's rows are heads, 2 = its columns are
    auto padded = [&](long long x) { const long long hd = x / dm, j = x % dm; return hd * d + (j < dm / 2 ? j : d / 2 + j - dm / 2); };
    if (head_pad == 1) dr = dst_row0 + padded(r);
    if (head_pad == 2) dc = padded(c);
    elem<DT>::st(dst + (size_t)(dr * dst_ld + dc), v);
}

int launch_convert_slice(Launcher &L, int src_dtype, const void *src, int64_t src_ld, int64_t r0, int64_t c0,
                         int64_t rows, int64_t cols, int dst_dtype, void *dst, int64_t dst_ld, int64_t dst_row0,
                         int row_mode, int head_pad, int64_t dm, int64_t d, int via_bf16) {
    const int64_t total = rows * cols;
    const unsigned blocks = (unsigned)((total + 255) / 256);
    if (dst_dtype == FL_DTYPE_BF16)
        return L.launch(KC_CONVERT, 0, 0, convert_slice_kernel<bf16_t>, dim3(blocks), dim3(256), 0, src, src_dtype,
                        (long long)src_ld, (long long)r0, (long long)c0, (long long)rows, (long long)cols,
                        (bf16_t *)dst, (long long)dst_ld, (long long)dst_row0, row_mode, head_pad, (int)dm, (int)d, 0);
    return L.launch(KC_CONVERT, 0, 0, convert_slice_kernel<float>, dim3(blocks), dim3(256), 0, src, src_dtype,
                    (long long)src_ld, (long long)r0, (long long)c0, (long long)rows, (long long)cols, (float *)dst,
                    (long long)dst_ld, (long long)dst_row0, row_mode, head_pad, (int)dm, (int)d, via_bf16);
}

int launch_convert_vec_f32(Launcher &L, int src_dtype, const void *src, int64_t off, int64_t n, float *dst) {
    return launch_convert_slice(L, src_dtype, src, n + off, 0, off, 1, n, FL_DTYPE_F32, dst, n, 0, 0);
}

}  // namespace fl
