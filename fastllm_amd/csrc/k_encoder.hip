// k_encoder.hip -- the kernels of the BERT / MiniLM encoder forward (the reference's MiniLMModel, src/models/embeddings.rs) that the
// decoder never needed: LayerNorm with bias fused with the embedding sum (:370-378) and with the residual adds (:185-190, :236-241),
// bias + GELU (:229-231), unmasked softmax attention over a ragged batch (:155-166) and masked-mean pooling + L2 norm (:341-368).
// The projections are launch_linear's (k_linear.hip).
//
// Every buffer is PACKED: the sequences of a call lie back to back, sequence s owns rows [offsets[s], offsets[s + 1]).  No kernel
// here forms a sum over rows of two sequences, and every reduction has a fixed order, so a sequence's result does not depend on its
// neighbours in the batch.
#include "kernels.h"
#include "attn_mfma.h"

namespace fl {

// ------------------------------------------------------------------------------- LayerNorm (one wave per row)
// candle_nn::LayerNorm: mean and biased variance over h in fp32, (x - mean) / sqrt(var + eps) * w + b.  The lane has just written
// the pre-norm values of ITS chunks (lane, lane + 64, ...) to xr and passes their sum; it reads the same chunks back (its own
// stores, so they are visible to it) for the variance and for the output: any h, no register array.
template <typename OT>
__device__ inline void ln_finish(float *xr, float sum, const float *__restrict__ w, const float *__restrict__ b, float eps, OT *xn, int h,
                                 int lane) {
    const float mean = wave_sum(sum) / (float)h;
    float sq = 0.f;
    for (int c = lane; c * 8 < h; c += 64) {
        float v[8];
        load8(xr + c * 8, v);
#pragma unroll
        for (int j = 0; j < 8; j++) { const float dl = v[j] - mean; sq = fmaf(dl, dl, sq); }
    }
    const float sd = sqrtf(wave_sum(sq) / (float)h + eps);
    for (int c = lane; c * 8 < h; c += 64) {
        float v[8], wv[8], bv[8], o[8];
        load8(xr + c * 8, v);
        load8(w + c * 8, wv);
        load8(b + c * 8, bv);
#pragma unroll
        for (int j = 0; j < 8; j++) o[j] = (v[j] - mean) / sd * wv[j] + bv[j];
        store8(xr + c * 8, o);
        store8(xn + c * 8, o);
    }
}

// x = LN(word[id] + pos[t - offsets[s]] (+ token-type row 0)): embed_tokens (:370-378); eps is the caller's (1e-12, :317)
template <typename CT>
__global__ __launch_bounds__(256) void encoder_embed_ln_kernel(const CT *__restrict__ word, const CT *__restrict__ pos, const CT *__restrict__ tt0,
                                                               const uint32_t *__restrict__ ids, const int32_t *__restrict__ row_seq,
                                                               const int32_t *__restrict__ offsets, const float *__restrict__ w,
                                                               const float *__restrict__ b, float eps, float *x_res, CT *xn, int T, int h) {
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (r >= T) return;
    const CT *wr = word + (size_t)ids[r] * h;
    const CT *pr = pos + (size_t)(r - offsets[row_seq[r]]) * h;
    float *xr = x_res + (size_t)r * h;
    float sum = 0.f;
    for (int c = lane; c * 8 < h; c += 64) {
        float a[8], p[8];
        load8(wr + c * 8, a);
        load8(pr + c * 8, p);
#pragma unroll
        for (int j = 0; j < 8; j++) a[j] += p[j];
        if (tt0) {
            load8(tt0 + c * 8, p);
#pragma unroll
            for (int j = 0; j < 8; j++) a[j] += p[j];
        }
#pragma unroll
        for (int j = 0; j < 8; j++) sum += a[j];
        store8(xr + c * 8, a);
    }
    ln_finish(xr, sum, w, b, eps, xn + (size_t)r * h, h, lane);
}

int launch_encoder_embed_ln(Launcher &L, int dtype, const void *word, const void *pos, const void *tt0, const uint32_t *ids,
                            const int32_t *row_seq, const int32_t *offsets, const float *w, const float *b, float eps, float *x_res, void *xn,
                            int64_t T, int64_t h) {
    if (h % 8) FL_FAIL(FL_ERR_UNSUPPORTED, "encoder_embed_ln: hidden_size must be a multiple of 8");
    const double es = dtype == FL_DTYPE_BF16 ? 2 : 4, bytes = (double)T * h * (2 * es + 3 * 4 + es);
    const dim3 grid((unsigned)((T + 3) / 4));
    if (dtype == FL_DTYPE_BF16)
        return L.launch(KC_ENC_EMBED_LN, bytes, 0, encoder_embed_ln_kernel<bf16_t>, grid, dim3(256), 0, (const bf16_t *)word, (const bf16_t *)pos,
                        (const bf16_t *)tt0, ids, row_seq, offsets, w, b, eps, x_res, (bf16_t *)xn, (int)T, (int)h);
    return L.launch(KC_ENC_EMBED_LN, bytes, 0, encoder_embed_ln_kernel<float>, grid, dim3(256), 0, (const float *)word, (const float *)pos,
                    (const float *)tt0, ids, row_seq, offsets, w, b, eps, x_res, (float *)xn, (int)T, (int)h);
}

// x = LN(x + (sum of the projection's split-K slabs, in slab order, + its bias)): the residual adds of :185-190 and :236-241
template <typename OT>
__global__ __launch_bounds__(256) void encoder_add_ln_kernel(float *x_res, const float *__restrict__ delta, int n_slab, long long slab_stride,
                                                             const float *__restrict__ bias, const float *__restrict__ w,
                                                             const float *__restrict__ b, float eps, OT *xn, int T, int h) {
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (r >= T) return;
    float *xr = x_res + (size_t)r * h;
    const float *dr = delta + (size_t)r * h;
    float sum = 0.f;
    for (int c = lane; c * 8 < h; c += 64) {
        float v[8], d[8], t[8];
        load8(xr + c * 8, v);
        load8(dr + c * 8, d);
        for (int sl = 1; sl < n_slab; sl++) {
            load8(dr + (size_t)sl * slab_stride + c * 8, t);
#pragma unroll
            for (int j = 0; j < 8; j++) d[j] += t[j];
        }
        if (bias) {
            load8(bias + c * 8, t);
#pragma unroll
            for (int j = 0; j < 8; j++) d[j] += t[j];
        }
#pragma unroll
        for (int j = 0; j < 8; j++) { v[j] += d[j]; sum += v[j]; }
        store8(xr + c * 8, v);
    }
    ln_finish(xr, sum, w, b, eps, xn + (size_t)r * h, h, lane);
}

int launch_encoder_add_ln(Launcher &L, int dtype, float *x_res, const float *delta, int n_slab, int64_t slab_stride, const float *bias,
                          const float *w, const float *b, float eps, void *xn, int64_t T, int64_t h) {
    if (h % 8 || n_slab < 1) FL_FAIL(FL_ERR_UNSUPPORTED, "encoder_add_ln: hidden_size must be a multiple of 8");
    const double bytes = (double)T * h * (4.0 * (4 + n_slab) + (dtype == FL_DTYPE_BF16 ? 2 : 4));
    const dim3 grid((unsigned)((T + 3) / 4));
    if (dtype == FL_DTYPE_BF16)
        return L.launch(KC_ENC_ADD_LN, bytes, 0, encoder_add_ln_kernel<bf16_t>, grid, dim3(256), 0, x_res, delta, n_slab, (long long)slab_stride,
                        bias, w, b, eps, (bf16_t *)xn, (int)T, (int)h);
    return L.launch(KC_ENC_ADD_LN, bytes, 0, encoder_add_ln_kernel<float>, grid, dim3(256), 0, x_res, delta, n_slab, (long long)slab_stride, bias,
                    w, b, eps, (float *)xn, (int)T, (int)h);
}

// ------------------------------------------------------------------------------- bias + GELU
// candle's Tensor::gelu is the tanh form, gelu_erf the exact one [UPSTREAM-RECALLED].  tanhf / erff in fp32, no fast-math forms:
// the fp32 mode is the parity mode.
__device__ inline float enc_act(float v, int act) {
    if (act == ENC_ACT_GELU_TANH) return 0.5f * v * (1.0f + tanhf(0.7978845608028654f * v * (1.0f + 0.044715f * v * v)));
    if (act == ENC_ACT_GELU_ERF) return 0.5f * v * (1.0f + erff(v * 0.7071067811865476f));
    return v;
}

template <typename OT>
__global__ __launch_bounds__(256) void encoder_bias_act_kernel(const float *__restrict__ y, int n_slab, long long slab_stride,
                                                               const float *__restrict__ bias, int act, OT *__restrict__ out, long long chunks,
                                                               int cpr /* chunks per row */) {
    const long long c = (long long)blockIdx.x * 256 + threadIdx.x;
    if (c >= chunks) return;
    float v[8], t[8];
    load8(y + c * 8, v);
    for (int sl = 1; sl < n_slab; sl++) {
        load8(y + (size_t)sl * slab_stride + c * 8, t);
#pragma unroll
        for (int j = 0; j < 8; j++) v[j] += t[j];
    }
    if (bias) {
        load8(bias + (c % cpr) * 8, t);
#pragma unroll
        for (int j = 0; j < 8; j++) v[j] += t[j];
    }
#pragma unroll
    for (int j = 0; j < 8; j++) v[j] = enc_act(v[j], act);
    store8(out + c * 8, v);
}

int launch_encoder_bias_act(Launcher &L, int dtype, const float *y, int n_slab, int64_t slab_stride, const float *bias, int act, void *out,
                            int64_t T, int64_t N) {
    if (N % 8 || n_slab < 1) FL_FAIL(FL_ERR_UNSUPPORTED, "encoder_bias_gelu: the row width must be a multiple of 8");
    const long long chunks = (long long)T * (N / 8);
    const double bytes = (double)T * N * (4.0 * n_slab + (dtype == FL_DTYPE_BF16 ? 2 : 4));
    const dim3 grid((unsigned)((chunks + 255) / 256));
    if (dtype == FL_DTYPE_BF16)
        return L.launch(KC_ENC_BIAS_ACT, bytes, 0, encoder_bias_act_kernel<bf16_t>, grid, dim3(256), 0, y, n_slab, (long long)slab_stride, bias,
                        act, (bf16_t *)out, chunks, (int)(N / 8));
    return L.launch(KC_ENC_BIAS_ACT, bytes, 0, encoder_bias_act_kernel<float>, grid, dim3(256), 0, y, n_slab, (long long)slab_stride, bias, act,
                    (float *)out, chunks, (int)(N / 8));
}

// ------------------------------------------------------------------------------- attention, bf16 (MFMA)
// One workgroup = (sequence, head, 64 query rows): four waves of 16 query rows each run attn_mfma.h's 32-key step
// (v_mfma_f32_16x16x32_bf16 for Q K^T and P V, fp32 accumulators, online softmax, probabilities rounded to bf16) over the keys of
// THIS sequence only.  A K tile [32 keys][D] and a V^T tile [D][32 keys] are staged in LDS in LdsKV's swizzled format and shared by
// the four waves; V is transposed on the way in (the packed buffer is row-major).  Rows of the last key tile at or beyond the
// sequence's length are staged as zeros and masked (attn_tile: key < len); query rows beyond it are computed on zeros and not
// written.  The loads below never touch a row outside [offsets[s], offsets[s + 1]).
template <int D>
__global__ __launch_bounds__(256) void encoder_attention_mfma_kernel(const bf16_t *__restrict__ q, const bf16_t *__restrict__ k,
                                                                     const bf16_t *__restrict__ v, int ld, const int32_t *__restrict__ offsets,
                                                                     float scale, bf16_t *__restrict__ out, int ldo) {
    __shared__ __attribute__((aligned(16))) unsigned char kt[32 * D * 2];
    __shared__ __attribute__((aligned(16))) unsigned char vt[D * 64];
    const int s = blockIdx.x, head = blockIdx.y, q0 = blockIdx.z * 64;
    const int r0 = offsets[s], len = offsets[s + 1] - r0;
    if (q0 >= len) return;                                         // (the whole workgroup: the grid is sized for the longest sequence)
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, i = lane & 15, g4 = lane >> 4;
    const int qrow = q0 + wave * 16 + i;
    bf16x8 qf[D / 32];
#pragma unroll
    for (int dk = 0; dk < D / 32; dk++) {
        uint4v z = {0u, 0u, 0u, 0u};
        if (qrow < len) z = *reinterpret_cast<const uint4v *>(q + (size_t)(r0 + qrow) * ld + head * D + dk * 32 + g4 * 8);
        qf[dk] = __builtin_bit_cast(bf16x8, z);
    }
    MfmaAttnState<D> st;
    st.init();
    const LdsKV<D> kv{kt, vt, i, g4};
    constexpr int CPR = D / 8;
    for (int kbase = 0; kbase < len; kbase += 32) {
        for (int c = tid; c < 32 * CPR; c += 256) {
            const int row = c / CPR, ch = c % CPR;
            uint4v kk = {0u, 0u, 0u, 0u}, vv = {0u, 0u, 0u, 0u};
            if (kbase + row < len) {
                const size_t g = (size_t)(r0 + kbase + row) * ld + head * D + ch * 8;
                kk = *reinterpret_cast<const uint4v *>(k + g);
                vv = *reinterpret_cast<const uint4v *>(v + g);
            }
            *reinterpret_cast<uint4v *>(kt + row * (D * 2) + ((ch ^ (row & (CPR - 1))) << 4)) = kk;
#pragma unroll
            for (int e = 0; e < 8; e++) {
                const int dr = ch * 8 + e;
                *reinterpret_cast<bf16_t *>(vt + dr * 64 + (((row >> 3) ^ ((dr >> 2) & 3)) << 4) + (row & 7) * 2) =
                    (bf16_t)((vv[e >> 1] >> ((e & 1) * 16)) & 0xffffu);
            }
        }
        __syncthreads();
        attn_tile<D>(st, qf, kv, kbase, len, 0, 0, scale, lane);
        __syncthreads();
    }
    float lt = st.l;                                               // partial in the four lane groups of a query column
    lt += __shfl_xor(lt, 16, 64);
    lt += __shfl_xor(lt, 32, 64);
    float lq[4];
#pragma unroll
    for (int r = 0; r < 4; r++) lq[r] = __shfl(lt, 4 * g4 + r, 64);
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const int row = q0 + wave * 16 + 4 * g4 + r;
        if (row < len) {
            bf16_t *o = out + (size_t)(r0 + row) * ldo + head * D + i;
#pragma unroll
            for (int db = 0; db < D / 16; db++) o[db * 16] = float_to_bf16_bits(st.O[db][r] / lq[r]);
        }
    }
}

// ------------------------------------------------------------------------------- attention, fp32 (VALU; the parity mode)
// One wave per query row: lane j takes keys j, j + 64, ... of the row's own sequence with its own online softmax (expf, scores
// DIVIDED by sqrt(d) as in :158); the lanes' states are merged in a fixed butterfly order.
template <int D>
__global__ __launch_bounds__(256) void encoder_attention_f32_kernel(const float *__restrict__ q, const float *__restrict__ k,
                                                                    const float *__restrict__ v, int ld, const int32_t *__restrict__ offsets,
                                                                    float *__restrict__ out, int ldo) {
    const int s = blockIdx.x, head = blockIdx.y, lane = threadIdx.x & 63;
    const int r0 = offsets[s], len = offsets[s + 1] - r0;
    const int qrow = blockIdx.z * 4 + (threadIdx.x >> 6);
    if (qrow >= len) return;
    float qv[D], o[D];
    const float *qp = q + (size_t)(r0 + qrow) * ld + head * D;
#pragma unroll
    for (int c = 0; c < D / 4; c++) {
        const float4v t = *reinterpret_cast<const float4v *>(qp + c * 4);
#pragma unroll
        for (int j = 0; j < 4; j++) { qv[c * 4 + j] = t[j]; o[c * 4 + j] = 0.f; }
    }
    const float sqrt_d = sqrtf((float)D);
    float m = -INFINITY, l = 0.f;
    for (int key = lane; key < len; key += 64) {
        const float *kp = k + (size_t)(r0 + key) * ld + head * D, *vp = v + (size_t)(r0 + key) * ld + head * D;
        float sc = 0.f;
#pragma unroll
        for (int c = 0; c < D / 4; c++) {
            const float4v t = *reinterpret_cast<const float4v *>(kp + c * 4);
#pragma unroll
            for (int j = 0; j < 4; j++) sc = fmaf(qv[c * 4 + j], t[j], sc);
        }
        sc /= sqrt_d;
        const float mn = fmaxf(m, sc), a = expf(m - mn), p = expf(sc - mn);
        l = l * a + p;
#pragma unroll
        for (int c = 0; c < D / 4; c++) {
            const float4v t = *reinterpret_cast<const float4v *>(vp + c * 4);
#pragma unroll
            for (int j = 0; j < 4; j++) o[c * 4 + j] = fmaf(p, t[j], o[c * 4 + j] * a);
        }
        m = mn;
    }
    const float mw = wave_max(m);
    const float f = m == -INFINITY ? 0.f : expf(m - mw);             // a lane that saw no key contributes nothing
    const float lw = wave_sum(l * f);
    float mine = 0.f;
#pragma unroll
    for (int j = 0; j < D; j++) {
        const float t = wave_sum(o[j] * f);
        if (lane == j) mine = t;
    }
    if (lane < D) out[(size_t)(r0 + qrow) * ldo + head * D + lane] = mine / lw;
}

bool encoder_attention_supported(int64_t d) { return d == 32 || d == 64; }

int launch_encoder_attention(Launcher &L, int dtype, const void *q, const void *k, const void *v, int64_t ld, const int32_t *offsets, int64_t n_seq,
                             int64_t max_len, int64_t T_total, int64_t H, int64_t d, float scale, void *out) {
    if (!encoder_attention_supported(d)) FL_FAIL(FL_ERR_UNSUPPORTED, "encoder attention: head_dim %lld (32 or 64)", (long long)d);
    if (ld % 8 || ld < H * d || n_seq < 1 || max_len < 1 || H < 1 || H > 65535 || max_len > 65535 * 4)
        FL_FAIL(FL_ERR_BAD_ARGUMENT, "encoder attention: bad shape");
    const double es = dtype == FL_DTYPE_BF16 ? 2 : 4;
    const double bytes = (double)T_total * H * d * 4 * es, flops = 4.0 * (double)T_total * max_len * H * d;     // (flops: an upper bound for a ragged batch)
    const int ldo = (int)(H * d);
    if (dtype == FL_DTYPE_BF16) {
        const dim3 grid((unsigned)n_seq, (unsigned)H, (unsigned)((max_len + 63) / 64));
        if (d == 64)
            return L.launch(KC_ENC_ATTN, bytes, flops, encoder_attention_mfma_kernel<64>, grid, dim3(256), 0, (const bf16_t *)q, (const bf16_t *)k,
                            (const bf16_t *)v, (int)ld, offsets, scale, (bf16_t *)out, ldo);
        return L.launch(KC_ENC_ATTN, bytes, flops, encoder_attention_mfma_kernel<32>, grid, dim3(256), 0, (const bf16_t *)q, (const bf16_t *)k,
                        (const bf16_t *)v, (int)ld, offsets, scale, (bf16_t *)out, ldo);
    }
    const dim3 grid((unsigned)n_seq, (unsigned)H, (unsigned)((max_len + 3) / 4));
    if (d == 64)
        return L.launch(KC_ENC_ATTN, bytes, flops, encoder_attention_f32_kernel<64>, grid, dim3(256), 0, (const float *)q, (const float *)k,
                        (const float *)v, (int)ld, offsets, (float *)out, ldo);
    return L.launch(KC_ENC_ATTN, bytes, flops, encoder_attention_f32_kernel<32>, grid, dim3(256), 0, (const float *)q, (const float *)k,
                    (const float *)v, (int)ld, offsets, (float *)out, ldo);
}

// ------------------------------------------------------------------------------- pooling
// mean_pooling with the all-ones mask (:346-368) and normalize_l2 (:341-344): one workgroup per sequence, a thread per column walks the
// sequence's rows in order; the sum of squares is reduced in a fixed order.
__global__ __launch_bounds__(256) void encoder_pool_l2_kernel(const float *__restrict__ x, const int32_t *__restrict__ offsets, int h,
                                                              float *__restrict__ out) {
    __shared__ float red[4];
    const int s = blockIdx.x, tid = threadIdx.x;
    const int r0 = offsets[s], len = offsets[s + 1] - r0;
    float sq = 0.f;
    for (int c = tid; c < h; c += 256) {
        float a = 0.f;
        for (int r = 0; r < len; r++) a += x[(size_t)(r0 + r) * h + c];
        a /= (float)len;
        out[(size_t)s * h + c] = a;
        sq = fmaf(a, a, sq);
    }
    sq = wave_sum(sq);
    if ((tid & 63) == 0) red[tid >> 6] = sq;
    __syncthreads();
    const float nrm = sqrtf(red[0] + red[1] + red[2] + red[3]);
    for (int c = tid; c < h; c += 256) out[(size_t)s * h + c] /= nrm;      // (the thread's own earlier stores)
}

int launch_encoder_pool_l2(Launcher &L, const float *x, const int32_t *offsets, int64_t n_seq, int64_t h, float *out) {
    return L.launch(KC_ENC_POOL, 0, 0, encoder_pool_l2_kernel, dim3((unsigned)n_seq), dim3(256), 0, x, offsets, (int)h, out);
}

}  // namespace fl
