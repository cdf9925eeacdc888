// k_linear.hip -- projection kernels: y = x . W^T (+bias) for the QKV / O / gate-up / down /
// lm_head matmuls of the decoder (candle Linear::forward).
//
//   gemv_kernel      T == 1 (decode): the HBM-bound weight stream (k_gemv.hip).
//   gemm_generic     any T, any shape: 64x64 LDS-tiled fp32-FMA kernel (fp32 parity mode and odd
//                    shapes).
//   gemm_mfma        T > 1, bf16: MFMA-tiled kernel (k_gemm_mfma.hip).
#include <stdlib.h>

#include <atomic>

#include <algorithm>

#include "kernels.h"

namespace fl {


// =============================================================================== generic GEMM
// 64x64 output tile, 16-deep K slices through LDS (as fp32), 256 threads, 4x4 per thread with
// column stride 16 so that a thread owns gate column c and up column c+16 of the interleaved
// gate/up layout.  Any T, N, K.
template <typename WT, typename XT>
__global__ __launch_bounds__(256) void gemm_generic_kernel(const WT *__restrict__ W, const XT *__restrict__ X,
                                                           const float *__restrict__ bias, void *__restrict__ out,
                                                           int T, int N, int K, int epi,
                                                           const float *__restrict__ row_scale) {
    __shared__ float xs[16][64 + 1];
    __shared__ float ws[16][64 + 1];
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    const int m0 = blockIdx.y * 64, n0 = blockIdx.x * 64;
    float acc[4][4] = {};
    for (int k0 = 0; k0 < K; k0 += 16) {
        for (int i = threadIdx.x; i < 64 * 16; i += 256) {
            int r = i >> 4, kk = i & 15;
            int m = m0 + r, n = n0 + r, k = k0 + kk;
            xs[kk][r] = (m < T && k < K) ? elem<XT>::ld(X + (size_t)m * K + k) : 0.f;
            ws[kk][r] = (n < N && k < K) ? elem<WT>::ld(W + (size_t)n * K + k) : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < 16; kk++) {
            float a[4], b[4];
#pragma unroll
            for (int i = 0; i < 4; i++) { a[i] = xs[kk][ty * 4 + i]; b[i] = ws[kk][tx + 16 * i]; }
#pragma unroll
            for (int i = 0; i < 4; i++)
#pragma unroll
                for (int j = 0; j < 4; j++) acc[i][j] = fmaf(a[i], b[j], acc[i][j]);
        }
        __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < 4; i++) {
        int m = m0 + ty * 4 + i;
        if (m >= T) continue;
        if (row_scale) {
            const float rs = row_scale[m];
#pragma unroll
            for (int j = 0; j < 4; j++) acc[i][j] *= rs;
        }
        if (epi == EPI_GATEUP) {
#pragma unroll
            for (int j = 0; j < 4; j += 2) {
                int n = n0 + tx + 16 * j;                 // gate column; up is n + 16
                if (n + 16 < N) {
                    int q = (n >> 5) * 16 + (n & 15);
                    float gt = acc[i][j], up = acc[i][j + 1];
                    float a = gt / (1.0f + expf(-gt)) * up;
                    elem<XT>::st(reinterpret_cast<XT *>(out) + (size_t)m * (N / 2) + q, a);
                }
            }
        } else {
#pragma unroll
            for (int j = 0; j < 4; j++) {
                int n = n0 + tx + 16 * j;
                if (n < N) reinterpret_cast<float *>(out)[(size_t)m * N + n] = acc[i][j] + (bias ? bias[n] : 0.f);
            }
        }
    }
}

template <typename WT, typename XT>
static int launch_gemm_generic(Launcher &L, const void *W, const void *x, const float *bias, void *y,
                               int64_t T, int64_t N, int64_t K, int epi, const float *row_scale) {
    dim3 grid((unsigned)((N + 63) / 64), (unsigned)((T + 63) / 64));
    double bytes = (double)N * K * sizeof(WT) + (double)T * K * sizeof(XT);
    return L.launch(KC_GEMM_GENERIC, bytes, 2.0 * T * N * K, gemm_generic_kernel<WT, XT>, grid, dim3(256), 0,
                    (const WT *)W, (const XT *)x, bias, y, (int)T, (int)N, (int)K, epi, row_scale);
}

// ================================================================================ the planner
static bool kernel_reads_rs_parts(int kernel) {
    return kernel == LK_H4 || kernel == LK_W14 || kernel == LK_SKF || kernel == LK_8P || kernel == LK_4W_ROPE;
}
// a captured launch is never a sliced 128 x 256 one (its host-side word set would be baked into the graph)
static bool h4_ok(int ks, bool captured) { return ks > 0 && !(captured && ks > 1); }
static LinearPlan finish(LinearPlan p, int dtype, int64_t T, int64_t N) {
    // (every launch of the plan must take the sums; a peeled matrix is kept on the vector.  FL_DEBUG_RS_PARTS, tests: every bf16
    // prompt projection is planned as reading them, so that kernels which take a vector meet them)
    p.reads_rs_parts = (kernel_reads_rs_parts(p.kernel) && p.n_main == N && (p.rows_main == T || kernel_reads_rs_parts(p.rest))) ||
                       (dtype == FL_DTYPE_BF16 && T > 1 && !tune(TK_FORCE_GENERIC_GEMM) && tune(TK_DEBUG_RS_PARTS));
    return p;
}

// The tiled kernels (k_gemm_mfma.hip): K slabs, whole-matrix stream-K, a column-peeled matrix (whole rounds of 256 x 256 tiles, the rest
// on the 128 x 256 kernel, in stream-K form or on the smaller tiles), or one grid of the kernel the cost model picks.
static void plan_tiles(LinearPlan &p, int64_t T, int64_t N, int64_t K, int epi, bool bias, int max_split, bool takes_slabs, bool captured) {
    p.ks = p.n_split = (takes_slabs && !bias) ? gemm_mfma_ksplit(T, N, K, epi, max_split) : 1;
    int64_t n_main = 0;
    if (p.ks == 1 && gemm_streamk_whole(T, N, K)) {
        p.kernel = LK_8P_STREAMK;
    } else if (p.ks == 1 && gemm_peel_plan(T, N, K, &n_main)) {
        p.kernel = gemm_tile_kernel(T, n_main, K, epi, bias, 1, true);
        p.n_main = n_main;
        const int ks = captured ? 0 : gemm_h4_tail_slices(T, N - n_main, K);
        p.tail = ks ? LK_H4 : tune(TK_GEMM_STREAMK) ? LK_8P_STREAMK : gemm_tile_kernel(T, N - n_main, K, epi, bias, 1, false);
        p.tail_ks = std::max(ks, 1);
    } else {
        p.kernel = gemm_tile_kernel(T, N, K, epi, bias, p.ks, true);
    }
}

LinearPlan plan_linear(int dtype, int64_t T, int64_t N, int64_t K, int epi, int tp, int max_split, bool bias, bool takes_slabs, bool captured) {
    LinearPlan p;
    p.n_main = N; p.rows_main = T;
    const bool generic = tune(TK_FORCE_GENERIC_GEMM) != 0;
    if (dtype == FL_DTYPE_F32) {
        p.kernel = T == 1 && gemv_supported(dtype, N, K) ? LK_GEMV : !generic && gemv_f32_rows_supported(T, N, K, epi) ? LK_F32_ROWS :
                   !generic && gemm_f32_mfma_supported(T, N, K) ? LK_F32_MFMA : LK_GENERIC;
        return p;
    }
    if (dtype != FL_DTYPE_BF16) return p;
    if (T == 1 && gemv_supported(dtype, N, K)) { p.kernel = LK_GEMV; return finish(p, dtype, T, N); }
    if (!generic && T > 1) {
        // mid-size prompts: 128 x 256 tiles, K slices summed inside the launch (k_gemm_h4.hip) -- one complete output, no slabs
        int ks = gemm_h4_plan(T, N, K, epi);
        // a tensor-parallel rank's projections (no slabs: the all-reduce wants the sum): K slices that meet inside the launch
        if (!h4_ok(ks, captured) && tp > 1 && max_split <= 1) ks = gemm_h4_plan_whole(T, N, K, epi);
        if (h4_ok(ks, captured)) { p.kernel = LK_H4; p.ks = ks; return finish(p, dtype, T, N); }
        // a few tokens past an even number of 256-row tiles: 3 x 128 tiles are a round and a half of the chip and cost two (Mistral-7B gate/up
        // 512 / 513 tokens: 92.6 / 170.3 us).  The even part keeps its whole rounds and the last rows go as a launch of their own on
        // whatever serves that many rows (ring kernel 36-46 us up to 32 rows, short-prompt GEMM 47-56 us up to 128).  Whole Mistral-7B
        // prefills, split / one launch: 513 tokens 10.25 / 10.87 ms, 545 10.76 / 11.01, 600 11.26 / 11.37, 1025 16.49 / 16.83, 1100
        // 16.91 / 17.08 -- and 700 12.48 / 12.29, 768 12.68 / 12.50, 1280 18.46 / 18.17: the second weight pass stops paying near 100 rows
        if (epi == EPI_GATEUP && T > 512 && tune(TK_GATEUP_ROWSPLIT) && !bias) {
            const int64_t tm = (T + 255) / 256, T0 = (tm - 1) * 256;
            if ((tm & 1) && T - T0 <= 96 && gemm_w14_plan(T0, N, K, epi)) {
                const LinearPlan r = plan_linear(dtype, T - T0, N, K, epi, tp, max_split, bias, false, captured);
                p.kernel = LK_W14; p.rows_main = T0; p.rest = r.kernel; p.rest_ks = r.ks;
                return finish(p, dtype, T, N);
            }
        }
        // 224-column tiles where they fill the chip and 256-column ones do not (k_gemm_w14.hip)
        if (gemm_w14_plan(T, N, K, epi)) { p.kernel = LK_W14; return finish(p, dtype, T, N); }
    }
    // short prompts / decode batches on the kernel whose K slices meet inside the launch (k_gemm_skf.hip): a tensor-parallel rank's
    // complete outputs (no slabs for its all-reduce) up to 64 rows -- tp = 4, 32 rows: down_proj 22.6 -> 11.6 us, 128 rows: o_proj
    // 11.1 -> 18.1 (the last arriver's tail grows with the tile) --; gate/up of the opt-in five-launch layer; every shape when forced
    if (!generic && T > 1 && T <= 128) {
        const int skf = tune(TK_GEMM_SKF);
        const bool whole = epi == EPI_F32 && ((skf >= 1 && tp > 1 && max_split <= 1 && T <= 64) || skf >= 3);
        if ((epi == EPI_GATEUP && skf >= 2) || whole) {
            const int ks = gemm_skf_plan(T, N, K, epi);
            if (ks > 0 && (ks > 1 || epi == EPI_GATEUP || skf >= 3)) { p.kernel = LK_SKF; p.ks = ks; return finish(p, dtype, T, N); }
        }
    }
    // prompts of 2-32 tokens: the wide gate/up stream on the LDS-DMA ring kernel of the decode batches (5.8 / 5.3 TB/s at <= 16 / 32 rows against 4.9)
    if (!generic && T > 1 && T <= 32 && epi == EPI_GATEUP && N >= 8192 && tune(TK_PREFILL_DMA) && gemv_dma_supported((int)T, N, K, epi, 0) &&
        gemv_dma_ksplit(K, 0, epi) == 1) {
        p.kernel = LK_DMA;
    } else if (!generic && tune(TK_GEMM_SKINNY) && gemm_skinny_supported(T, N, K)) {     // short prompts: a weight stream
        p.kernel = LK_SKINNY;   // (more slabs cost the summing launch more than they save here)
        p.ks = p.n_split = (takes_slabs && !bias) ? gemm_skinny_ksplit(T, N, K, epi, std::min(max_split, 4)) : 1;
    } else if (!generic && gemm_mfma_supported(dtype, T, N, K)) {
        plan_tiles(p, T, N, K, epi, bias, max_split, takes_slabs, captured);
    } else {
        p.kernel = LK_GENERIC;
    }
    return finish(p, dtype, T, N);
}

// Long prompts on the 256 x 256 kernel whole (a peeled matrix: + a stream-K tail) or, from 257 tokens of the models' widths, the
// 128 x 256 kernel in 2-4 in-launch K slices (gemm_h4_plan); short ones on k_gemm_skf.hip when opted in.
LinearPlan plan_resid(int dtype, int64_t T, int64_t N, int64_t K, int max_split, bool captured) {
    LinearPlan p;
    p.n_main = N; p.rows_main = T;
    if (tune(TK_GEMM_RESID) == 0 || dtype != FL_DTYPE_BF16) return p;
    int ks = tune(TK_GEMM_SKF) >= 2 ? gemm_skf_plan(T, N, K, EPI_RESID) : 0;
    if (ks > 0) { p.kernel = LK_SKF; p.ks = ks; return p; }
    ks = N % 16 == 0 ? gemm_h4_plan(T, N, K, EPI_RESID) : 0;
    if (h4_ok(ks, captured)) { p.kernel = LK_H4; p.ks = ks; return p; }
    if (tune(TK_GEMM_8P) != 1 || T < 256 || K % 64 || K / 64 < 2 || N % 16 || gemm_streamk_whole(T, N, K)) return p;
    int64_t n_main = 0;
    if (gemm_peel_plan(T, N, K, &n_main)) {                           // main launch + a tail, both with the residual epilogue
        if (!tune(TK_GEMM_STREAMK)) return p;
        p.kernel = LK_8P; p.n_main = n_main;
        ks = captured ? 0 : gemm_h4_tail_slices(T, N - n_main, K);
        p.tail = ks ? LK_H4 : LK_8P_STREAMK; p.tail_ks = std::max(ks, 1);
    } else if (gemm_pick_kernel(T, N, K, 1) == LK_8P && gemm_resid_8p_wins(T, N, K, max_split)) {
        p.kernel = LK_8P;
    }
    return p;
}

// The RoPE / bias / KV-append epilogue rides in the QKV projection where a kernel has it -- short prompts on k_gemm_skf.hip (opt-in),
// mid-size ones (and a tensor-parallel rank's narrower q | k | v) on k_gemm_h4.hip, long ones on the four-wave 256 x 256 kernel where
// launch_linear would run ONE plain grid of 256 x 256 tiles, or whole rounds + tail columns on the 128 x 256 kernel (1, 2 or 4 in-launch
// slices) -- so no fp32 QKV matrix exists.  Otherwise the plain projection: K slabs and stream-K pieces keep the fp32 output and the
// rope_kv launch (which sums the slabs anyway).
LinearPlan plan_qkv_rope(int dtype, int64_t T, int64_t N, int64_t K, int64_t d, int64_t kv_width, int tp, int max_split) {
    LinearPlan p;
    p.n_main = N; p.rows_main = T; p.rope = true;
    if (dtype == FL_DTYPE_BF16) {
        int h4 = gemm_h4_plan(T, N, K, EPI_QKV_ROPE);
        if (!h4 && tp > 1 && kv_width % 128 == 0 && N % 128 == 0) h4 = gemm_h4_plan_whole(T, N, K, EPI_QKV_ROPE);
        const int skf = !h4 && tp == 1 && tune(TK_GEMM_SKF) >= 2 ? gemm_skf_plan(T, N, K, EPI_QKV_ROPE, (int)d) : 0;
        if (skf || h4) { p.kernel = skf ? LK_SKF : LK_H4; p.ks = skf ? skf : h4; return finish(p, dtype, T, N); }
        if (tune(TK_GEMM_ROPE_4W) && T >= 768 && !tune(TK_FORCE_GENERIC_GEMM) && tune(TK_GEMM_8P) == 1 && gemm_mfma_supported(dtype, T, N, K) &&
            !gemm_streamk_whole(T, N, K)) {
            int64_t nm = N;
            int ks = 0;
            const bool ok = gemm_peel_plan(T, N, K, &nm) ? (ks = gemm_h4_tail_slices(T, N - nm, K)) && ks != 3 && nm % 128 == 0 && (N - nm) % 128 == 0
                                                        : gemm_mfma_ksplit(T, N, K, EPI_F32, max_split) == 1 && gemm_pick_kernel(T, N, K, 1) == LK_8P;
            if (ok && gemm_4w_rope_supported(T, nm, K) && gemm_4w_rule(T, nm, K, K / 64, false)) {
                p.kernel = LK_4W_ROPE; p.n_main = nm;
                if (nm < N) { p.tail = LK_H4; p.tail_ks = ks; }
                return finish(p, dtype, T, N);
            }
        }
    }
    return plan_linear(dtype, T, N, K, EPI_F32, tp, max_split, false, true, false);
}

// ================================================================================ carrying a plan out
// One launch over rows [0, T) and the column range [0, N) of an output whose rows are ldc elements apart.  A kernel that takes its
// row scales as a vector finishes partial sums the caller left first (rs_parts_to_vector).
static int launch_one(Launcher &L, int kernel, int ks, int dtype, const void *W, const void *x, const float *bias, void *y, int64_t T, int64_t N,
                      int64_t K, int epi, const float *row_scale, int64_t ldc, const ResidEpi *re, const RopeEpi *ro) {
    if (!kernel_reads_rs_parts(kernel)) FL_TRY(rs_parts_to_vector(L, row_scale, T));
    switch (kernel) {
    case LK_GEMV: {
        GemvArgs a; a.W = W; a.x = x; a.bias = bias; a.out = y; a.N = (int)N; a.K = (int)K; a.epi = epi; a.pro = PRO_X; a.x_scale = row_scale;
        return launch_gemv(L, dtype, a);
    }
    case LK_H4: return launch_gemm_h4(L, W, x, bias, y, T, N, K, epi, row_scale, ks, ldc, re, ro);
    case LK_W14: return launch_gemm_w14(L, W, x, bias, y, T, N, K, epi, row_scale, ldc);
    case LK_SKF: return launch_gemm_skf(L, W, x, bias, y, T, N, K, epi, row_scale, ks, re, ro);
    case LK_DMA: {
        GemvBatchArgs a; a.W = W; a.x = x; a.x_scale = row_scale; a.out = y; a.N = (int)N; a.K = (int)K; a.epi = epi; a.pro = PRO_X; a.B = (int)T; a.nks = 1;
        return launch_gemv_dma(L, a);
    }
    case LK_SKINNY: return launch_gemm_skinny(L, W, x, bias, y, T, N, K, epi, row_scale, ks);
    case LK_8P: return launch_gemm_8p(L, W, x, bias, y, T, N, K, epi, row_scale, ks, ldc, false, re);
    case LK_8P_STREAMK: return launch_gemm_8p(L, W, x, bias, y, T, N, K, epi, row_scale, 1, ldc, true, re);
    case LK_256: case LK_128: return launch_gemm_mfma(L, kernel == LK_256, W, x, bias, y, T, N, K, epi, row_scale, ks, ldc);
    case LK_4W_ROPE: return launch_gemm_4w_rope(L, W, x, bias, T, N, K, row_scale, *ro);
    case LK_GENERIC:
        if (dtype == FL_DTYPE_F32) return launch_gemm_generic<float, float>(L, W, x, bias, y, T, N, K, epi, row_scale);
        return launch_gemm_generic<bf16_t, bf16_t>(L, W, x, bias, y, T, N, K, epi, row_scale);
    case LK_F32_ROWS: return launch_gemv_f32_rows(L, W, x, bias, y, T, N, K, epi, row_scale);
    case LK_F32_MFMA: return launch_gemm_f32_mfma(L, W, x, bias, y, T, N, K, epi, row_scale);
    }
    FL_FAIL(FL_ERR_UNSUPPORTED, "no kernel planned for this projection (dtype %d)", dtype);
}

int launch_plan(Launcher &L, const LinearPlan &p, int dtype, const void *W, const void *x, const float *bias, void *y, int64_t T, int64_t N,
                int64_t K, int epi, const float *row_scale, const ResidEpi *re, const RopeEpi *ro) {
    FL_TRY(launch_one(L, p.kernel, p.ks, dtype, W, x, bias, y, p.rows_main, p.n_main, K, epi, row_scale, N, re, ro));
    if (p.n_main < N) {     // a peeled matrix's tail: the same rows, the output's later columns
        const int64_t c = p.n_main;
        ResidEpi rt; RopeEpi ot;
        if (re) { rt = *re; rt.h += c; rt.w += c; rt.xn = (bf16_t *)rt.xn + c; rt.part += (c / 256) * 4; }
        if (ro) { ot = *ro; ot.col_base = (int)c; }
        void *yt = y ? (char *)y + (size_t)(epi == EPI_GATEUP ? c / 2 * 2 : c * 4) : nullptr;
        FL_TRY(launch_one(L, p.tail, p.tail_ks, dtype, (const bf16_t *)W + (size_t)c * K, x, bias ? bias + c : nullptr, yt, p.rows_main, N - c, K, epi,
                          row_scale, N, re ? &rt : nullptr, ro ? &ot : nullptr));
    }
    if (p.rows_main < T) {  // a gate/up row split: the last rows, all columns
        const int64_t r = p.rows_main;
        Launcher L2 = L;
        if (L2.rsp.part) L2.rsp.part += (size_t)r * L2.rsp.np;
        FL_TRY(launch_one(L2, p.rest, p.rest_ks, dtype, W, (const char *)x + (size_t)r * K * 2, bias, (char *)y + (size_t)r * (N / 2) * 2, T - r, N, K,
                          epi, row_scale ? row_scale + r : nullptr, N, re, ro));
    }
    return FL_OK;
}

int launch_linear(Launcher &L, int dtype, const void *W, const void *x, const float *bias, void *y,
                  int64_t T, int64_t N, int64_t K, int epi, const float *row_scale, int max_split, int *n_split_out, bool captured) {
    if (n_split_out) *n_split_out = 1;
    if (T <= 0 || N <= 0 || K <= 0) FL_FAIL(FL_ERR_BAD_ARGUMENT, "launch_linear: bad shape");
    if (epi == EPI_GATEUP && N % 32) FL_FAIL(FL_ERR_BAD_ARGUMENT, "gate/up matrix rows must be a multiple of 32");
    const LinearPlan p = plan_linear(dtype, T, N, K, epi, L.tp, max_split, bias != nullptr, n_split_out != nullptr, captured);
    if (n_split_out) *n_split_out = p.n_split;
    return launch_plan(L, p, dtype, W, x, bias, y, T, N, K, epi, row_scale);
}

}  // namespace fl
