// gemv_parts.h -- what the decode weight streams have in common apart from the stream itself: the row map of the paired
// layouts, the fused RMSNorm prologue and the epilogues.  gemv_kernel (k_gemv.hip), gemv_w8_kernel (k_gemv_w8.hip), eng_stream
// (k_engine.hip) and the two batch kernels (k_gemv_batch.hip) are written in terms of these; each keeps its own load_next /
// consume loop.  Two places keep text of their own because the compiler's register allocation was worse through this header
// (profiles/gemv_parts/README.md): gemv_kernel's norm prologue, and the QKV row map and store of gemv_batch_mfma_kernel.  Everything here is a template or an inline function over compile-time EPI / R, so an instantiation pays
// registers only for the epilogue it has.
#pragma once
#include "kernels.h"

namespace fl {

// Weight row r of row group g (R rows per group).  EPI_GATEUP: the 16-interleaved layout -- channel q's gate row and its up
// row 16 further; EPI_QKV_ROPE: the rotate-half partners j, j + d/2 of a head; else consecutive rows.
template <int EPI, int R>
__device__ inline int gemv_row_of(int g, int r, int d, int half) {
    if constexpr (EPI == EPI_GATEUP) {
        const int q = g * (R / 2) + (r >> 1);
        return (q >> 4) * 32 + (q & 15) + ((r & 1) << 4);
    } else if constexpr (EPI == EPI_QKV_ROPE) {
        const int q = g * (R / 2) + (r >> 1);
        const int hd = q / half, j = q - hd * half;
        return hd * d + j + (r & 1) * half;
    } else {
        return g * R + r;
    }
}

// candle silu(g) * u
__device__ inline float gemv_silu_gate(float gt, float up) { return gt / (1.0f + expf(-gt)) * up; }

// EPI_GATEUP: channel q = g * R/2 + r/2 of `out` from the group's gate and up sums (lane 0)
template <typename XT, int R>
__device__ inline void gemv_store_gateup(XT *out, int N, int g, const float (&sum)[R]) {
#pragma unroll
    for (int r = 0; r < R; r += 2)
        if (gemv_row_of<EPI_GATEUP, R>(g, r + 1, 0, 0) < N) elem<XT>::st(out + g * (R / 2) + (r >> 1), gemv_silu_gate(sum[r], sum[r + 1]));
}

// q and k heads take the rotate-half RoPE (App. A.4), value heads go out as they are
__device__ inline bool qkv_rotates(int hd, int H, int Hkv) { return hd < H + Hkv; }

// Where the QKV projection's rows go: head hd < H to the q buffer, the next Hkv heads to slot `slot` of the K cache
// [Hkv][seq][d], the last Hkv to the value cache -- transposed [Hkv][d][v_ld] (v_ld > 0) or laid out as K.
template <typename XT>
struct QkvDest {
    XT *q, *k, *v;                   // q rows of this sequence; the layer's cache bases
    int H, Hkv, d;
    size_t seq, v_ld;
    template <typename A>            // GemvArgs / EngArgs: one sequence, the layer's caches as given
    __device__ static QkvDest of_args(const A &a) {
        return {reinterpret_cast<XT *>(a.q_out), reinterpret_cast<XT *>(a.k_cache), reinterpret_cast<XT *>(a.v_cache), a.H, a.Hkv, a.d,
                (size_t)a.max_seq, a.v_ld > 0 ? (size_t)a.v_ld : (size_t)0};
    }
    // sequence b of a batch: its own caches (V always transposed), the layer found through kv_layer_off
    __device__ static QkvDest of_seq(const GemvBatchArgs &a, const SeqRef &sq, int b) {
        return {reinterpret_cast<XT *>(a.q_out) + (size_t)b * a.H * a.d, reinterpret_cast<XT *>(sq.k) + a.kv_layer_off * sq.seq_alloc,
                reinterpret_cast<XT *>(sq.v) + a.kv_layer_off * sq.seq_alloc, a.H, a.Hkv, a.d, (size_t)sq.seq_alloc, (size_t)sq.seq_alloc};
    }
    // channel 0 of head hd at `slot`; `stride`: elements between channels j and j + 1
    __device__ XT *at(int hd, uint32_t slot, size_t &stride) const {
        stride = 1;
        if (hd < H) return q + (size_t)hd * d;
        if (hd < H + Hkv) return k + ((size_t)(hd - H) * seq + slot) * d;
        if (v_ld > 0) { stride = v_ld; return v + (size_t)(hd - H - Hkv) * d * v_ld + slot; }
        return v + ((size_t)(hd - H - Hkv) * seq + slot) * d;
    }
    // the pair (j, j + half) of head hd, rotated by the caller where qkv_rotates(hd)
    __device__ void store_pair(int hd, int j, int half, uint32_t slot, float x0, float x1) const {
        size_t stride;
        XT *dst = at(hd, slot, stride);
        elem<XT>::st(dst + (size_t)j * stride, x0);
        elem<XT>::st(dst + (size_t)(j + half) * stride, x1);
    }
};

// EPI_QKV_ROPE of a single-sequence stream (fused K4/K5): the operands of a row group's pairs are REQUESTED when the group
// starts -- position from the step state, then cos / sin and the bias of the pair's two rows (Qwen2) -- so that their two
// dependent round trips overlap the weight stream instead of trailing it.  (R + 1) / 2 pairs: eng_stream also exists with R = 1.
template <typename XT, int R>
struct GemvRope {
    static constexpr int NP = (R + 1) / 2;
    QkvDest<XT> to;
    const float *cos_tab, *sin_tab, *bias;
    int N, half;
    uint32_t p = 0, slot = 0;
    float c[NP], s[NP], b0[NP], b1[NP];

    template <typename A>
    __device__ GemvRope(const A &a, const float *bias_, int N_)
        : to(QkvDest<XT>::of_args(a)), cos_tab(a.cos_tab), sin_tab(a.sin_tab), bias(bias_), N(N_), half(a.d >> 1) {}
    __device__ void begin(const StepState *st, int max_pos) {
        const uint32_t pos = st->pos;
        slot = st->len;
        p = pos < (uint32_t)max_pos ? pos : (uint32_t)max_pos - 1;
    }
    __device__ void prefetch(int g) {
#pragma unroll
        for (int r = 0; r < R; r += 2) {
            const int q = g * (R / 2) + (r >> 1);
            const int hd = q / half, j = q - hd * half;
            const bool rot = qkv_rotates(hd, to.H, to.Hkv);
            c[r >> 1] = rot ? cos_tab[(size_t)p * half + j] : 1.f;
            s[r >> 1] = rot ? sin_tab[(size_t)p * half + j] : 0.f;
            const int r0w = gemv_row_of<EPI_QKV_ROPE, R>(g, r, to.d, half), r1w = gemv_row_of<EPI_QKV_ROPE, R>(g, r + 1, to.d, half);
            b0[r >> 1] = bias && r1w < N ? bias[r0w] : 0.f;                        // requested with the tables: in the epilogue it was a
            b1[r >> 1] = bias && r1w < N ? bias[r1w] : 0.f;                        //  round trip at the very end of the launch
        }
    }
    __device__ void store(int g, const float (&sum)[R]) const {                     // lane 0
#pragma unroll
        for (int r = 0; r < R; r += 2) {
            if (gemv_row_of<EPI_QKV_ROPE, R>(g, r + 1, to.d, half) >= N) continue;
            const int q = g * (R / 2) + (r >> 1);
            const int hd = q / half, j = q - hd * half;
            float x0 = sum[r], x1 = sum[r + 1];
            if (bias) { x0 += b0[r >> 1]; x1 += b1[r >> 1]; }
            if (qkv_rotates(hd, to.H, to.Hkv)) {
                float t0, t1;
                rope_rotate(x0, x1, c[r >> 1], s[r >> 1], t0, t1);
                x0 = t0; x1 = t1;
            }
            to.store_pair(hd, j, half, slot, x0, x1);
        }
    }
};

// Running ArgMax of the rows a wave has stored (lane 0); ties -> the larger index, as argmax_last: select_advance_kernel
// reads the workgroups' candidates in place of the vocabulary and relies on exactly this rule.
struct GemvBest {
    float v = -INFINITY;
    int i = -1;
    __device__ void consider(float y, int row) {
        if (row >= 0 && (i < 0 || y > v || (y == v && row > i))) { v = y; i = row; }
    }
};

// EPI_F32: rows g * R .. of `out` (+ bias), each offered to `best` where the launch leaves candidates (lane 0)
template <int R>
__device__ inline void gemv_store_f32(float *out, const float *bias, int N, int g, const float (&sum)[R], bool track, GemvBest &best) {
#pragma unroll
    for (int r = 0; r < R; r++) {
        const int row = g * R + r;
        if (row < N) {
            const float y = sum[r] + (bias ? bias[row] : 0.f);
            out[row] = y;
            if (track) best.consider(y, row);
        }
    }
}

// The workgroup's candidate (GemvArgs::amax): lane 0 of each wave w0 <= w < w1 holds the best of its rows; cv / ci are LDS
// words indexed by wave.  Every thread of the workgroup calls this (barrier inside).
__device__ inline void gemv_leave_candidate(ArgmaxCand *amax, float *cv, int *ci, int w0, int w1, const GemvBest &best) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) { cv[wave] = best.v; ci[wave] = best.i; }
    __syncthreads();
    if (threadIdx.x == 0) {
        GemvBest b;
        for (int w = w0; w < w1; w++) b.consider(cv[w], ci[w]);
        amax[1 + blockIdx.x] = ArgmaxCand{b.v, b.i};
        if (blockIdx.x == 0) amax[0] = ArgmaxCand{0.f, (int)gridDim.x};
    }
}

// Prologue PRO_NORM (fused K2/K9, and K1 for layer 0) of a single-sequence stream.  RMSNorm is folded around the dot product,
//     W . (v / m * w)  =  (1/m) * W . (v * w),     v = x_in + delta (or the token's embedding row),
// so the workgroup stages x' = v * w in LDS with no dependence on m = sqrt(mean(v^2) + eps): the sum of squares rides along
// in the same pass and is combined behind the SAME barrier as the staging; the caller applies the returned 1/m to its
// accumulators.  Workgroup 0 also writes the updated residual v to x_out.  A thread holds NCH chunks of 8 in registers
// (blockDim.x * NCH * 8 >= K, host-checked); slot(c): element offset of chunk c in xs; start_stream() issues the first
// weight loads -- after the (short) activation loads so that the counted wait for those does not have to drain them, and
// before anything waits.  red: one LDS float per wave.  delta is ONE vector (GemvArgs::delta_nslab == 1, host-checked).
// gemv_kernel (k_gemv.hip) keeps a copy of this text, with the sliced delta: see there.  That leaves gemv_w8_kernel as the one
// caller today; the function stands here, with slot() and NCH open, as the prologue of the next single-sequence weight format.
template <int NCH, typename ET, typename XT, typename SlotF, typename StartF>
__device__ inline float gemv_norm_prologue(const GemvArgs &a, XT *xs, float *red, const SlotF &slot, const StartF &start_stream) {
    const int tid = threadIdx.x, nthr = blockDim.x, K = a.K, nchunk = K >> 3;
    float v[NCH][8], wn[NCH][8], dl[NCH][8];
    const ET *erow = nullptr;
    if (a.embed) erow = reinterpret_cast<const ET *>(a.embed) + (size_t)a.st->token * K;
#pragma unroll
    for (int i = 0; i < NCH; i++) {                  // requests only: nothing here waits (an add of delta in this loop made the
        const int c = tid + nthr * i;                //  weight stream below start a round trip late)
        if (c < nchunk) {
            if (erow) load8(erow + c * 8, v[i]); else load8(a.x_in + c * 8, v[i]);
            load8(a.norm_w + c * 8, wn[i]);
            if (a.delta) load8(a.delta + c * 8, dl[i]);
        }
    }
    start_stream();
    float ss = 0.f;
#pragma unroll
    for (int i = 0; i < NCH; i++) {
        const int c = tid + nthr * i;
        if (c < nchunk) {
            if (a.delta) {
#pragma unroll
                for (int j = 0; j < 8; j++) v[i][j] += dl[i][j];
            }
            float o[8];
#pragma unroll
            for (int j = 0; j < 8; j++) { ss = fmaf(v[i][j], v[i][j], ss); o[j] = v[i][j] * wn[i][j]; }
            store8(xs + slot(c), o);
            if (blockIdx.x == 0 && a.x_out) store8(a.x_out + c * 8, v[i]);
        }
    }
    ss = wave_sum(ss);
    if ((tid & 63) == 0) red[tid >> 6] = ss;
    __syncthreads();
    ss = 0.f;
    for (int w = 0; w < (nthr >> 6); w++) ss += red[w];
    return 1.0f / sqrtf(ss / (float)K + a.eps);          // candle rms_norm (App. A.2)
}

}  // namespace fl
