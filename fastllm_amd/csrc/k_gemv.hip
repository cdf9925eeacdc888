// k_gemv.hip -- the decode (T = 1) weight-streaming kernel: y = W[N,K] . x  with fused prologue
// and epilogues.  This is the dominant kernel of the hot path: 97.5 % of a decode step's HBM
// bytes are linear-layer weights read exactly once.
//
// Streaming (HBM-bound, cdna guide "GEMV / M <= 16" row): each wave owns R rows at a time and
// reads them 16 B per lane (1 KiB per wave instruction), non-temporal, straight to VGPRs -- no
// LDS round trip for read-once bytes.  bf16 weights: the wave's (row group, K block) items form
// ONE stream, a block (U chunks x R rows = 4 or 8 KiB) ahead in a second register buffer, every
// load unconditional so that hipcc keeps counted vmcnt waits; the arithmetic is v_dot2c_f32_bf16
// (common.h: inline asm, with the wait the gfx940+ dot-result hazard asks for behind every run
// of dots; tests/test_dot_hazard.py checks the shipped code objects).  A projection short enough
// for one row group per wave requests its whole share before the prologue (SMALL).  fp32 weights:
// straight-line blocks of U chunks x R rows with FMAs, the K tail as one more block.  8..12 waves
// per CU overlap each other's load and multiply phases, and the first block is requested BEFORE
// x is staged so HBM is busy during the prologue.  fp32 accumulate; 64-lane shuffle reduce.  x is
// staged once per workgroup in LDS (ds_read_b128).  Against a bare read stream of the same bytes
// (tools/micro/stream_ceiling.hip, 6.76 TB/s) the largest launch of a Mistral-7B step is 6 % slower.
//
// Geometry: one workgroup per CU (or two), 4..12 waves each, chosen so that every wave gets the
// same number of row groups (a ragged last round costs 1/rounds of the kernel) and everything is
// resident at once.
//
// Prologue PRO_NORM (fused K2/K9, and K1 for layer 0): RMSNorm is folded around the dot product,
//     W . (v / m * w)  =  (1/m) * W . (v * w),     v = x_in + delta (or the token's embedding row),
// so the workgroup stages x' = v * w in LDS with no dependence on m = sqrt(mean(v^2) + eps): the
// sum of squares rides along in the same pass and is combined behind the SAME barrier as the
// staging; 1/m is applied to the accumulator in the epilogue.  Workgroup 0 also writes the updated
// residual v to x_out (a different buffer than x_in: other workgroups still read x_in).
//
// Epilogue EPI_RESID + prologue PRO_XS (bf16): where gemv_resid_edge (gemv_geometry.h) says so, the o_proj / down_proj
// launch finishes what PRO_NORM redoes in every workgroup -- per row, on the lane that holds the row's sum: v = h_in + sum to h_out,
// bf16(v * w_next) to xs, and behind one barrier the fmaf chain over every 8 rows to cs -- and the launch behind the norm stages xs
// (one 16-byte chunk and one float per thread) and sums cs where PRO_NORM sums its own squares: the same chains, the same bits.
//
// Epilogues: EPI_F32 (+bias) -> fp32, or -- GemvArgs::ll, the row-parallel o_proj / down_proj of a tensor-parallel
// group -- summed over the ranks right here (comm_ll.h);  EPI_GATEUP: silu(gate)*up on the 16-interleaved layout;
// EPI_QKV_ROPE (fused K4/K5): rows are paired (j, j+d/2) per head, RoPE is applied with the
// position from the device step state and q / rotated k / v go straight to the q buffer and
// the KV cache slot `len`.
#include <stdlib.h>

#include <algorithm>
#include <atomic>
#include <type_traits>

#include "comm_ll.h"
#include "gemv_geometry.h"
#include "gemv_parts.h"
#include "kernels.h"

namespace fl {

constexpr int kGemvMaxThreads = 768;     // 12 waves: 170 VGPRs per lane available

template <typename WT> struct RawChunk { uint4v v[sizeof(WT) == 2 ? 1 : 2]; };

#ifndef FL_GEMV_DOT2
#define FL_GEMV_DOT2 1
#endif
constexpr bool kGemvDot2 = FL_GEMV_DOT2 != 0;
#ifndef FL_GEMV_PIPE
#define FL_GEMV_PIPE 1
#endif
constexpr bool kGemvPipe = FL_GEMV_PIPE != 0 && kGemvDot2;

#if !defined(FL_GEMV_PLAIN_LOADS) || !defined(FL_EXPERIMENTAL)
#undef FL_GEMV_PLAIN_LOADS
#define FL_GEMV_PLAIN_LOADS 0              // (-DFL_GEMV_PLAIN_LOADS=1, EXPERIMENTAL build only: the weight stream through plain instead of non-temporal loads)
#endif
__device__ inline void load_raw_nt(const bf16_t *p, RawChunk<bf16_t> &r) {
    if constexpr (FL_GEMV_PLAIN_LOADS != 0) r.v[0] = *reinterpret_cast<const uint4v *>(p);
    else r.v[0] = __builtin_nontemporal_load(reinterpret_cast<const uint4v *>(p));
}
__device__ inline void load_raw_nt(const float *p, RawChunk<float> &r) {
    r.v[0] = __builtin_nontemporal_load(reinterpret_cast<const uint4v *>(p));
    r.v[1] = __builtin_nontemporal_load(reinterpret_cast<const uint4v *>(p + 4));
}
__device__ inline void unpack_raw(const RawChunk<bf16_t> &r, float (&o)[8]) { unpack8(r.v[0], o); }
__device__ inline void unpack_raw(const RawChunk<float> &r, float (&o)[8]) {
#pragma unroll
    for (int i = 0; i < 4; i++) { o[i] = __uint_as_float(r.v[0][i]); o[4 + i] = __uint_as_float(r.v[1][i]); }
}

// MAXT = 768: up to 12 waves per workgroup (170 VGPRs per lane).
// SMALL: every wave owns at most ONE row group and K <= 2 blocks of U chunks (host-checked): the whole
// weight share of the wave (2*U*R KiB) is requested before x is staged -- one HBM round trip instead of
// two for the short QKV / o_proj launches, where ramp-up is most of the kernel.
template <typename WT, typename XT, int R, int U, int PRO, int MAXT, bool SMALL, int EPI, bool FUSE_AR>
__global__ __launch_bounds__(MAXT) void gemv_kernel(const GemvArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    __shared__ float red[kGemvMaxThreads / 64];
    __shared__ float cv[kGemvMaxThreads / 64];       // ArgMax candidates of the waves (GemvArgs::amax)
    __shared__ int ci[kGemvMaxThreads / 64];
    __shared__ float rv[EPI == EPI_RESID ? kGemvMaxThreads / 64 * R : 1];   // EPI_RESID: the rows the workgroup finished (v), [wave * R + r]
    XT *xs = reinterpret_cast<XT *>(lds_raw);
    const WT *__restrict__ W = reinterpret_cast<const WT *>(a.W);
    const int N = a.N, K = a.K;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nthr = blockDim.x, nwv = nthr >> 6;
    const int nchunk = K >> 3;                       // 8-element chunks; K % 8 == 0
    const int half = a.d >> 1;
    const int ngroups = (N + R - 1) / R;
    const int gw = blockIdx.x * nwv + wave, nw = gridDim.x * nwv;

    auto row_of = [&](int g, int r) -> int { return gemv_row_of<EPI, R>(g, r, a.d, half); };
    typedef RawChunk<WT> Buf[R][U];
    // first K block of this wave's first row group: requested before x is staged, so HBM is busy
    // during the prologue
    constexpr int NPRE = SMALL ? 2 : 1;              // K blocks requested ahead of the prologue
    Buf pre[NPRE];
    bool have_pre[NPRE];
#pragma unroll
    for (int i = 0; i < NPRE; i++) have_pre[i] = gw < ngroups && lane + 64 * (U * (i + 1) - 1) < nchunk;
    // PIPE (bf16, every launch that is not SMALL): the wave's (row group, K block) items form ONE stream, requested a block
    // ahead into two register buffers -- while a block is multiplied the next one is in flight, also across row groups and
    // their epilogues.  Every load of the stream is unconditional (no control flow around loads: hipcc then keeps COUNTED
    // vmcnt waits): past the end of K a lane re-reads the last chunk (its x is zeroed); the last one or two items are
    // peeled off the loop, so that the loop itself never requests past the wave's last item.
    constexpr bool PIPE = kGemvPipe && !SMALL && sizeof(WT) == 2 && sizeof(XT) == 2;
    const int wave_u = __builtin_amdgcn_readfirstlane(wave);                       // wave-uniform copies for the stream's bookkeeping
    const int gw_u = blockIdx.x * nwv + wave_u;
    const int nb = (nchunk + 64 * U - 1) / (64 * U);                                // K blocks per row group (the last may be partial)
    const int n_items = gw_u < ngroups ? (ngroups - gw_u + nw - 1) / nw * nb : 0;  // this wave's items
    int lg = gw_u, lb = 0;                                                          // load stream: next item = (row group, block)
    auto load_next = [&](Buf &buf) {
        const int g = min(lg, ngroups - 1);                                         // (a wave without work reads the last group's first block once)
#pragma unroll
        for (int r = 0; r < R; r++) {
            const int row = row_of(g, r);
            const WT *wr = W + (size_t)(row < N ? row : N - 1) * K;
#pragma unroll
            for (int u = 0; u < U; u++) load_raw_nt(wr + (size_t)min(lane + 64 * (U * lb + u), nchunk - 1) * 8, buf[r][u]);
        }
        if (++lb == nb) { lb = 0; lg += nw; }
    };
    constexpr bool kStraightPre = SMALL && (PRO == PRO_XS || EPI == EPI_RESID);
    const WT *wrow[R];                               // kStraightPre: this lane's first chunk of the wave's rows, worked out ahead of the prologue's requests
    if constexpr (kStraightPre) {
#pragma unroll
        for (int r = 0; r < R; r++) {
            const int row = row_of(gw, r);
            wrow[r] = W + (size_t)(row < N ? row : N - 1) * K + lane * 8;
        }
    }
    auto prefetch = [&]() {
        if constexpr (PIPE) { load_next(pre[0]); return; }
#pragma unroll
        for (int i = 0; i < NPRE; i++) {
            // PRO_XS / EPI_RESID: the first block goes out with no control flow around it (K >= one block: host-checked; a wave
            // without a row group re-reads the last row), so that the wait for the activations requested in front of it stays a
            // COUNTED one.  Behind a branch hipcc waits for the weights as well before x is staged: the stream's round trip and
            // the prologue then run one after the other.
            if (!(kStraightPre && i == 0) && !have_pre[i]) continue;
#pragma unroll
            for (int r = 0; r < R; r++) {
                if constexpr (kStraightPre) {
#pragma unroll
                    for (int u = 0; u < U; u++) load_raw_nt(wrow[r] + (size_t)(64 * (U * i + u)) * 8, pre[i][r][u]);
                } else {
                    const int row = row_of(gw, r);
                    const WT *wp = W + (size_t)(row < N ? row : N - 1) * K;
#pragma unroll
                    for (int u = 0; u < U; u++) load_raw_nt(wp + (size_t)(lane + 64 * (U * i + u)) * 8, pre[i][r][u]);
                }
            }
        }
    };
    // EPI_RESID: the wave's rows of the residual stream and of the next norm's weight, requested before anything else (one row
    // group per wave, the grid covers N exactly: host-checked), so that their round trip does not trail the stream
    float hin[R], wnx[R];
    if constexpr (EPI == EPI_RESID) {
#pragma unroll
        for (int r = 0; r < R; r++) { hin[r] = a.x_in[gw_u * R + r]; wnx[r] = a.norm_w[gw_u * R + r]; }
    }
    float inv_m = 1.0f;
    if constexpr (PRO == PRO_XS) {
        // The vector an EPI_RESID launch finished: thread c stages chunk c of bf16(v * w) and takes that chunk's sum of squares --
        // the fmaf chain thread c of PRO_NORM runs over the same eight v -- so everything from wave_sum on is PRO_NORM's text and
        // 1/m has PRO_NORM's bits.  One chunk per thread (nthr >= K / 8, host-checked); no residual write, no norm weight.
        static_assert(PRO != PRO_XS || sizeof(XT) == 2, "PRO_XS stages a bf16 vector");
        const XT *__restrict__ x = reinterpret_cast<const XT *>(a.x);
        // requests only, and no branch around them (a thread past the vector re-reads its last chunk): behind a branch the
        // loaded values meet a constant at the join, which is a use -- hipcc then waits for them before the weights go out
        const int cc = min(tid, nchunk - 1);
        __builtin_amdgcn_sched_barrier(0);               // (the row addresses above stay above)
        const uint4v xr = *reinterpret_cast<const uint4v *>(x + cc * 8);
        const float csv = a.cs[cc];
        // ... and the order pinned: activations, then the stream, then the first use.  Left to itself the scheduler puts the
        // stream's loads in front (loads return in order: x then waits for the weights) or the select below in front of the stream
        __builtin_amdgcn_sched_barrier(0);
        prefetch();
        __builtin_amdgcn_sched_barrier(0);
        if (tid < nchunk) *reinterpret_cast<uint4v *>(xs + tid * 8) = xr;
        float ss = tid < nchunk ? csv : 0.f;
        ss = wave_sum(ss);
        if (lane == 0) red[wave] = ss;
        __syncthreads();
        ss = 0.f;
        for (int w = 0; w < nwv; w++) ss += red[w];
        inv_m = 1.0f / sqrtf(ss / (float)K + a.eps);           // candle rms_norm (App. A.2)
    } else if constexpr (PRO == PRO_NORM) {
        // This is gemv_norm_prologue (gemv_parts.h) written out, plus the sliced delta: called through the header, the bf16 SMALL
        // forms (the default QKV / o_proj / down_proj launches) took 98-100 VGPRs instead of 94-96 -- 4 waves per SIMD instead of
        // 5 -- and three fp32 forms spilled 12-16 bytes more (profiles/gemv_parts/README.md)
        constexpr int NCH = SMALL ? 1 : 3;           // nthr * NCH * 8 >= K (host-checked)
        float v[NCH][8], wn[NCH][8], dl[NCH][8];
        const WT *erow = nullptr;
        if (a.embed) erow = reinterpret_cast<const WT *>(a.embed) + (size_t)a.st->token * K;
#pragma unroll
        for (int i = 0; i < NCH; i++) {                  // requests only: nothing here waits (an add of delta in this loop made the
            const int c = tid + nthr * i;                //  weight stream below start a round trip late)
            if (c < nchunk) {
                if (erow) load8(erow + c * 8, v[i]); else load8(a.x_in + c * 8, v[i]);
                load8(a.norm_w + c * 8, wn[i]);
                if (a.delta) {
                    load8(a.delta + c * 8, dl[i]);
                    for (int s0 = 1; s0 < a.delta_nslab; s0 += 7) {        // partial vectors of a K-sliced producer (the opt-in fused attention
                        float ds[7][8];                                     // + o_proj launch): up to seven per round trip, fixed order; this path
#pragma unroll                                                              // does wait before the weights are requested
                        for (int u = 0; u < 7; u++)
                            if (s0 + u < a.delta_nslab) load8(a.delta + (size_t)(s0 + u) * K + c * 8, ds[u]);
                        // slab by slab onto the residual, ((x + d0) + d1) + ... -- the order rmsnorm_add and the batched stream
                        // sum slabs in, so that the same slabs give the same residual bits on every path
                        if (s0 == 1) {
#pragma unroll
                            for (int j = 0; j < 8; j++) dl[i][j] = v[i][j] + dl[i][j];
                        }
#pragma unroll
                        for (int u = 0; u < 7; u++)
                            if (s0 + u < a.delta_nslab) {
#pragma unroll
                                for (int j = 0; j < 8; j++) dl[i][j] += ds[u][j];
                            }
                    }
                }
            }
        }
        // the weight stream starts now: issued after the (short) activation loads so that the counted
        // wait for those does not have to drain the long weight loads
        prefetch();
        float ss = 0.f;
#pragma unroll
        for (int i = 0; i < NCH; i++) {
            const int c = tid + nthr * i;
            if (c < nchunk) {
                if (a.delta) {
                    const bool folded = a.delta_nslab > 1;               // (several slabs: dl already holds x + their sum, above)
#pragma unroll
                    for (int j = 0; j < 8; j++) v[i][j] = folded ? dl[i][j] : v[i][j] + dl[i][j];
                }
                float o[8];
#pragma unroll
                for (int j = 0; j < 8; j++) { ss = fmaf(v[i][j], v[i][j], ss); o[j] = v[i][j] * wn[i][j]; }
                store8(xs + c * 8, o);
                if (blockIdx.x == 0 && a.x_out) store8(a.x_out + c * 8, v[i]);
            }
        }
        ss = wave_sum(ss);
        if (lane == 0) red[wave] = ss;
        __syncthreads();
        ss = 0.f;
        for (int w = 0; w < nwv; w++) ss += red[w];
        inv_m = 1.0f / sqrtf(ss / (float)K + a.eps);           // candle rms_norm (App. A.2)
    } else {
        const XT *__restrict__ x = reinterpret_cast<const XT *>(a.x);
        constexpr int NXR = 4;
        uint4v xr[NXR][sizeof(XT) == 2 ? 1 : 2];
        // stage x through registers: up to NXR chunks per thread are requested before the weights
#pragma unroll
        for (int i = 0; i < NXR; i++) {
            const int c = tid + nthr * i;
            if (c < nchunk) {
                xr[i][0] = *reinterpret_cast<const uint4v *>(x + c * 8);
                if constexpr (sizeof(XT) == 4) xr[i][1] = *reinterpret_cast<const uint4v *>(x + c * 8 + 4);
            }
        }
        if (a.x_scale) inv_m = *a.x_scale;
        prefetch();
#pragma unroll
        for (int i = 0; i < NXR; i++) {
            const int c = tid + nthr * i;
            if (c < nchunk) {
                *reinterpret_cast<uint4v *>(xs + c * 8) = xr[i][0];
                if constexpr (sizeof(XT) == 4) *reinterpret_cast<uint4v *>(xs + c * 8 + 4) = xr[i][1];
            }
        }
        for (int c = tid + NXR * nthr; c < nchunk; c += nthr) {        // very long K: the rest
            if constexpr (sizeof(XT) == 2) {
                *reinterpret_cast<uint4v *>(xs + c * 8) = *reinterpret_cast<const uint4v *>(x + c * 8);
            } else {
                *reinterpret_cast<float4v *>(xs + c * 8) = *reinterpret_cast<const float4v *>(x + c * 8);
                *reinterpret_cast<float4v *>(xs + c * 8 + 4) = *reinterpret_cast<const float4v *>(x + c * 8 + 4);
            }
        }
        __syncthreads();
    }

    float acc[R];
#pragma unroll
    for (int r = 0; r < R; r++) acc[r] = 0.f;

    // RoPE epilogue operands are requested up front (gemv_parts.h), and again whenever a row group starts
    GemvRope<XT, R> rope(a, a.bias, N);
    if constexpr (EPI == EPI_QKV_ROPE) {
        rope.begin(a.st, a.max_pos);
        if (gw < ngroups) rope.prefetch(gw);
    }

    GemvBest best;                                                                  // running ArgMax of this wave's rows (lane 0)
    auto finish_group = [&](int g) {
        float sum[R];
#pragma unroll
        for (int r = 0; r < R; r++) { sum[r] = wave_sum(acc[r]) * inv_m; acc[r] = 0.f; }
        if constexpr (FUSE_AR) {                           // row-parallel projection of a tensor-parallel group (EPI_F32, no bias: host-checked)
            ll_allreduce_rows<R>(a.ll, a.ll_slot, g * R, N, sum, reinterpret_cast<float *>(a.out), lane);
            return;
        }
        if (lane != 0) return;
        if constexpr (EPI == EPI_RESID) {
            // each row is finished once, here: the residual add (sum + 0.f: the bits the plain epilogue stores as delta, a -0 sum
            // included), the next norm's v * w in the conversion of store8, and v for the workgroup's chunk sums below
            uint32_t pk[R / 2];
#pragma unroll
            for (int r = 0; r < R; r++) {
                const float v = hin[r] + (sum[r] + 0.f);
                rv[wave * R + r] = v;
                a.x_out[g * R + r] = v;
                const uint32_t b = float_to_bf16_bits(v * wnx[r]);
                if (r & 1) pk[r >> 1] |= b << 16; else pk[r >> 1] = b;
            }
#pragma unroll
            for (int r = 0; r < R / 2; r++) reinterpret_cast<uint32_t *>(a.xs_out)[g * (R / 2) + r] = pk[r];
            return;
        }
        if constexpr (EPI == EPI_GATEUP) gemv_store_gateup<XT, R>(reinterpret_cast<XT *>(a.out), N, g, sum);
        else if constexpr (EPI == EPI_QKV_ROPE) rope.store(g, sum);
        else gemv_store_f32<R>(reinterpret_cast<float *>(a.out), a.bias, N, g, sum, a.amax != nullptr, best);
    };
    // what a workgroup does once its waves are through: the ArgMax candidate (EPI_F32 with GemvArgs::amax), or (EPI_RESID) the sums of
    // squares of its nwv * R rows (a multiple of 8, host-checked) in chunks of 8 -- ss = fmaf(v, v, ss) from 0 in element order,
    // the chain thread c of the PRO_NORM prologue runs over chunk c
    auto leave_candidate = [&]() {
        if constexpr (EPI == EPI_RESID) {
            __syncthreads();
            const int nch = (nwv * R) >> 3;
            if (tid < nch) {
                float ss = 0.f;
#pragma unroll
                for (int j = 0; j < 8; j++) ss = fmaf(rv[8 * tid + j], rv[8 * tid + j], ss);
                a.cs_out[blockIdx.x * nch + tid] = ss;
            }
            return;
        }
        if constexpr (EPI != EPI_F32 || FUSE_AR) return;
        if (a.amax) gemv_leave_candidate(a.amax, cv, ci, 0, nwv, best);              // (kernel argument: uniform)
    };
    auto fma_block = [&](const Buf &buf, int c0) {
#pragma unroll
        for (int u = 0; u < U; u++) {
            if constexpr (kGemvDot2 && sizeof(WT) == 2 && sizeof(XT) == 2) {
                // bf16 x bf16: four v_dot2c_f32_bf16 per 16 bytes of weights (exact products, fp32 accumulate) instead of eight
                // unpacks + eight FMAs -- the wave is back at its loads sooner
                const uint4v xr = *reinterpret_cast<const uint4v *>(xs + (c0 + 64 * u) * 8);
#pragma unroll
                for (int r = 0; r < R; r++)
#pragma unroll
                    for (int j = 0; j < 4; j++) acc[r] = dot2c_bf16(buf[r][u].v[0][j], xr[j], acc[r]);
            } else {
                float xv[8];
                load8(xs + (c0 + 64 * u) * 8, xv);
#pragma unroll
                for (int r = 0; r < R; r++) {
                    float wv[8];
                    unpack_raw(buf[r][u], wv);
#pragma unroll
                    for (int j = 0; j < 8; j++) acc[r] = fmaf(wv[j], xv[j], acc[r]);
                }
            }
        }
        if constexpr (kGemvDot2 && sizeof(WT) == 2 && sizeof(XT) == 2) {
#pragma unroll
            for (int r = 0; r < R; r++) dot2c_settle(acc[r]);
        }
    };

    if constexpr (SMALL) {
        if (gw < ngroups) {
#pragma unroll
            for (int i = 0; i < NPRE; i++)
                if (have_pre[i]) fma_block(pre[i], lane + 64 * U * i);
            finish_group(gw);
        }
        leave_candidate();
        return;
    }
    if constexpr (PIPE) {
        int cg = gw_u, cb = 0;                                                      // consume stream
        const bool ragged = nchunk % (64 * U) != 0;
        auto consume = [&](const Buf &buf) {
            if constexpr (EPI == EPI_QKV_ROPE) {
                if (cb == 0 && cg != gw_u) rope.prefetch(cg);
            }
            const int c0 = lane + 64 * U * cb;
            if (ragged && cb == nb - 1) {                                           // wave-uniform: the partial last block of K
#pragma unroll
                for (int u = 0; u < U; u++) {
                    const int ci = c0 + 64 * u;
                    uint4v xr = *reinterpret_cast<const uint4v *>(xs + min(ci, nchunk - 1) * 8);
                    if (ci >= nchunk) xr = uint4v{0u, 0u, 0u, 0u};
#pragma unroll
                    for (int r = 0; r < R; r++)
#pragma unroll
                        for (int j = 0; j < 4; j++) acc[r] = dot2c_bf16(buf[r][u].v[0][j], xr[j], acc[r]);
                }
#pragma unroll
                for (int r = 0; r < R; r++) dot2c_settle(acc[r]);
            } else {
                fma_block(buf, c0);
            }
            if (++cb == nb) { finish_group(cg); cb = 0; cg += nw; }
        };
        Buf nxt;
        int t = 0;
#pragma nounroll
        for (; t + 2 < n_items; t += 2) {
            load_next(nxt);
            consume(pre[0]);
            load_next(pre[0]);
            consume(nxt);
        }
        if (n_items - t == 2) { load_next(nxt); consume(pre[0]); consume(nxt); }
        else if (n_items - t == 1) consume(pre[0]);
        leave_candidate();
        return;
    }
#pragma nounroll
    for (int g = gw; g < ngroups; g += nw) {
        if constexpr (EPI == EPI_QKV_ROPE) {
            if (g != gw) rope.prefetch(g);
        }
        const WT *wp[R];
#pragma unroll
        for (int r = 0; r < R; r++) {
            const int row = row_of(g, r);
            wp[r] = W + (size_t)(row < N ? row : N - 1) * K;
        }
        int c0 = lane;
        if (g == gw) {
#pragma unroll
            for (int i = 0; i < NPRE; i++)
                if (have_pre[i]) { fma_block(pre[i], c0); c0 += 64 * U; }
        }
#pragma nounroll
        for (; c0 + 64 * (U - 1) < nchunk; c0 += 64 * U) {      // full blocks of U chunks: straight-line, counted waits
            Buf w;
#pragma unroll
            for (int u = 0; u < U; u++)
#pragma unroll
                for (int r = 0; r < R; r++) load_raw_nt(wp[r] + (size_t)(c0 + 64 * u) * 8, w[r][u]);
            fma_block(w, c0);
        }
        // K tail: the remaining 1..U-1 whole 64-lane chunks as ONE straight-line block (K = 3584, 5632,
        // 18944 ... all leave such a remainder), then a generic loop for a ragged last chunk
        // ... and the tensor-parallel slices (K = 1792, 4736, 896 ...) end in a PARTIAL 64-lane chunk: the lanes past
        // the end load a clamped (valid) address and contribute zeros, so the block stays straight-line as well
        {
            const int remaining = nchunk - (c0 - lane);          // wave-uniform
            const int nblk = (remaining + 63) >> 6;
            if (remaining > 0 && nblk < U) {
                auto tail_block = [&](auto TU) {
                    constexpr int NT = decltype(TU)::value;
                    RawChunk<WT> w[R][NT];
#pragma unroll
                    for (int u = 0; u < NT; u++) {
                        const int ci = c0 + 64 * u, cc = ci < nchunk ? ci : nchunk - 1;
#pragma unroll
                        for (int r = 0; r < R; r++) load_raw_nt(wp[r] + (size_t)cc * 8, w[r][u]);
                    }
#pragma unroll
                    for (int u = 0; u < NT; u++) {
                        const int ci = c0 + 64 * u;
                        const bool ok = ci < nchunk;
                        float xv[8];
                        load8(xs + (ok ? ci : nchunk - 1) * 8, xv);
#pragma unroll
                        for (int j = 0; j < 8; j++) xv[j] = ok ? xv[j] : 0.f;
#pragma unroll
                        for (int r = 0; r < R; r++) {
                            float wv[8];
                            unpack_raw(w[r][u], wv);
#pragma unroll
                            for (int j = 0; j < 8; j++) acc[r] = fmaf(wv[j], xv[j], acc[r]);
                        }
                    }
                    c0 += 64 * NT;
                };
                if (nblk == 1) tail_block(std::integral_constant<int, 1>{});
                else if (nblk == 2) tail_block(std::integral_constant<int, 2>{});
                else if (nblk == 3) tail_block(std::integral_constant<int, 3>{});
                else if (U > 4 && nblk == 4) tail_block(std::integral_constant<int, 4>{});
            }
        }
#pragma nounroll
        for (; c0 < nchunk; c0 += 64) {                          // ragged tail of K
            float xv[8];
            load8(xs + c0 * 8, xv);
#pragma unroll
            for (int r = 0; r < R; r++) {
                float wv[8];
                load8_nt(wp[r] + (size_t)c0 * 8, wv);
#pragma unroll
                for (int j = 0; j < 8; j++) acc[r] = fmaf(wv[j], xv[j], acc[r]);
            }
        }
        finish_group(g);
    }
    leave_candidate();
}

// forced grid / waves per workgroup (fl_tune "gemv_blocks" / "gemv_waves"; 0 = automatic).  Rows per wave pass and chunks per block
// are rows of the switch table (TK_GEMV_R, TK_GEMV_U): read per launch, so "reload_env" reaches them like every other switch.
static std::atomic<int> g_force_blocks{0}, g_force_waves{0};

void gemv_set_tuning(int blocks, int waves) {
    if (blocks >= 0) g_force_blocks = blocks;
    if (waves >= 0) g_force_waves = waves;
}

bool gemv_supported(int dtype, int64_t N, int64_t K) {
    (void)N;
    if (dtype != FL_DTYPE_BF16 && dtype != FL_DTYPE_F32) return false;
    size_t lds = (size_t)K * (dtype == FL_DTYPE_BF16 ? 2 : 4);
    return K % 8 == 0 && K >= 8 && lds <= 160 * 1024 - 256;
}
// fused-norm prologue: every staging thread holds at most 3 chunks of 8 in registers, and the
// smallest workgroup is 256 threads
bool gemv_norm_supported(int dtype, int64_t N, int64_t K) { return gemv_supported(dtype, N, K) && K <= 6144; }

// the grid of an N x K launch with R rows per group (gemv_geometry.h), under the fl_tune grid
static GemvGeometry tuned_geometry(int64_t N, int64_t K, int R, size_t es) {
    return gemv_geometry((N + R - 1) / R, ((size_t)K * es + 15) & ~(size_t)15, device_cu_count(), g_force_blocks.load(), g_force_waves.load());
}

template <typename WT, typename XT, int R, int U, int PRO, int MAXT, bool SMALL, int EPI, bool FUSE_AR = false>
static int launch_gemv_ke(Launcher &L, const GemvArgs &a, int blocks, int waves, size_t lds) {
    auto kern = gemv_kernel<WT, XT, R, U, PRO, MAXT, SMALL, EPI, FUSE_AR>;
    FL_TRY(raise_dynamic_lds(reinterpret_cast<const void *>(kern), lds));
    double bytes = (double)a.N * a.K * sizeof(WT);
    char tag[32];
    // ",norm": the launch applies an RMSNorm to its input, through either prologue.  The recorded kernel lists
    // (tests/golden/kernel_selection.json) know a decode step's launches by these names, so the form an edge took shows only on
    // request -- fl_tune "gemv_resid" = 2: ",xs" for the staged-vector prologue, ",resid" for the producer
    const bool forms = tune(TK_GEMV_RESID) >= 2;
    snprintf(tag, sizeof tag, "%dx%d%s%s", a.N, a.K, PRO == PRO_XS && forms ? ",xs" : (PRO != PRO_X ? ",norm" : ""),
             a.epi == EPI_GATEUP ? ",glu" : (a.epi == EPI_QKV_ROPE ? ",rope" : (a.epi == EPI_RESID && forms ? ",resid" : "")));
    Launcher LL = L; LL.tag = tag;
    return LL.launch(KC_GEMV, bytes, 2.0 * a.N * a.K, kern, dim3((unsigned)blocks), dim3((unsigned)waves * 64), lds, a);
}

template <typename WT, typename XT, int R, int U, int PRO, int MAXT, bool SMALL>
static int launch_gemv_k(Launcher &L, const GemvArgs &a, int blocks, int waves, size_t lds) {
    if (a.epi == EPI_RESID) {                               // (bf16, plain prologue: launch_gemv has checked)
        if constexpr (sizeof(WT) == 2 && PRO == PRO_X) return launch_gemv_ke<WT, XT, R, U, PRO, MAXT, SMALL, EPI_RESID>(L, a, blocks, waves, lds);
        else FL_FAIL(FL_ERR_UNSUPPORTED, "launch_gemv: the residual epilogue is a bf16 launch with the plain prologue");
    }
    if (a.epi == EPI_GATEUP) return launch_gemv_ke<WT, XT, R, U, PRO, MAXT, SMALL, EPI_GATEUP>(L, a, blocks, waves, lds);
    if (a.epi == EPI_QKV_ROPE) return launch_gemv_ke<WT, XT, R, U, PRO, MAXT, SMALL, EPI_QKV_ROPE>(L, a, blocks, waves, lds);
    if constexpr (PRO != PRO_XS) {                          // (no tensor-parallel form of the staged-vector prologue)
        if (a.ll) return launch_gemv_ke<WT, XT, R, U, PRO, MAXT, SMALL, EPI_F32, true>(L, a, blocks, waves, lds);
    }
    return launch_gemv_ke<WT, XT, R, U, PRO, MAXT, SMALL, EPI_F32>(L, a, blocks, waves, lds);
}

template <typename WT, typename XT, int R, int U, int PRO>
static int launch_gemv_t(Launcher &L, const GemvArgs &a) {
    const int64_t N = a.N, K = a.K;
    size_t lds = ((size_t)K * sizeof(XT) + 15) & ~(size_t)15;
    const int64_t ngroups = (N + R - 1) / R;
    const GemvGeometry geo = tuned_geometry(N, K, R, sizeof(XT));
    int blocks = geo.blocks, waves = geo.waves;
    if (a.amax && blocks + 1 > kMaxArgmaxCand) {           // (callers ask gemv_leaves_candidates first; a tuned grid may still get here)
        FL_FAIL(FL_ERR_BAD_ARGUMENT, "launch_gemv: %d workgroups exceed the ArgMax candidate buffer (gemv_leaves_candidates not consulted)", blocks);
    }
    if (PRO == PRO_NORM && (int64_t)waves * 64 * 3 * 8 < K) waves = (int)((K + 64 * 3 * 8 - 1) / (64 * 3 * 8));   // staging capacity
    if (waves < 4) waves = 4;
    if (PRO == PRO_XS && (int64_t)waves * 64 < (K >> 3)) FL_FAIL(FL_ERR_UNSUPPORTED, "launch_gemv: %d threads stage fewer than K / 8 = %d chunks", waves * 64, (int)(K >> 3));
    if (a.epi == EPI_RESID) {
        // each row finished once by the wave that holds its sum, a workgroup's rows whole chunks of 8 (gemv_resid_edge, gemv_geometry.h)
        if (g_force_blocks.load() != 0 || g_force_waves.load() != 0) FL_FAIL(FL_ERR_UNSUPPORTED, "launch_gemv: the residual epilogue does not run on a forced grid");
        if ((int64_t)blocks * waves * R != N || (waves * R) % 8 != 0)
            FL_FAIL(FL_ERR_UNSUPPORTED, "launch_gemv: the residual epilogue needs a grid that covers N = %d exactly (%d x %d waves x %d rows)", (int)N, blocks, waves, R);
    }
    const int allow_small = tune(TK_GEMV_SMALL);
    const bool small = allow_small && sizeof(WT) == 2 && ngroups <= (int64_t)blocks * waves && (K >> 3) % (64 * U) == 0 &&
                       (K >> 3) <= 2 * 64 * U && (PRO != PRO_NORM || (int64_t)waves * 64 * 8 >= K);
    if constexpr (sizeof(WT) == 2) {                        // (fp32 weights never take the SMALL form: it is not instantiated for them)
        if (small) return launch_gemv_k<WT, XT, R, U, PRO, 768, true>(L, a, blocks, waves, lds);
    }
    return launch_gemv_k<WT, XT, R, U, PRO, 768, false>(L, a, blocks, waves, lds);
}

template <typename WT, typename XT, int PRO>
static int launch_gemv_ru(Launcher &L, const GemvArgs &a) {
    int R = tune(TK_GEMV_R), U = tune(TK_GEMV_U);
    // default (no FL_GEMV_U / fl_tune): four 1-KiB chunks in flight per row, two for the plain and RoPE epilogues at
    // K <= 4096 (Mistral-7B: o_proj 7.96 -> 7.48 us, lm_head 43.8 -> 42.0, QKV 11.95 -> 11.82; down_proj at K = 14336
    // 19.9 vs 20.9 and gate/up 38.2 vs 38.1 stay on four)
    if (U <= 0) {
        // fp32 weights: two 2-KiB chunks per row -- the four-chunk instantiations spill 20-48 VGPRs under the 168-register cap of a
        // 768-thread workgroup (Mistral-7B fp32 decode: gate/up 5.11 -> 5.41 TB/s, down_proj 5.03 -> 5.69, step 6.12 -> 5.78 ms)
        U = 2;
        // bf16 (two register buffers of the stream, dot2 arithmetic: 152-166 VGPRs at U = 8, no spills): 8 KiB per row group
        // and request round from K = 4096 (Mistral-7B: down_proj 19.9 -> 19.05 us, the others equal or better), 4 below
        if (sizeof(WT) == 2) U = (a.K >> 3) >= 512 ? 8 : 4;
        // the QKV projection is short enough for every wave to own ONE row group: with U = K / 512 its whole share is one block,
        // requested before the norm prologue runs (the SMALL form): Mistral-7B 11.8 -> 10.5 us
        // (bf16 only: with fp32 weights eight chunks per row are 128 VGPRs of stream buffers -- the fp32 mode's QKV ran at 1.4 TB/s from scratch spills)
        if (sizeof(WT) == 2 && R == 2 && a.epi == EPI_QKV_ROPE && a.pro != PRO_X && (a.K == 4096 || a.K == 3584)) U = a.K / 512;
    }
    if (R == 4 && U == 2) return launch_gemv_t<WT, XT, 4, 2, PRO>(L, a);
    if (R == 2 && U == 7) return launch_gemv_t<WT, XT, 2, 7, PRO>(L, a);
    if (R == 2 && U == 8) return launch_gemv_t<WT, XT, 2, 8, PRO>(L, a);
    if (R == 2 && U == 2) return launch_gemv_t<WT, XT, 2, 2, PRO>(L, a);
    return launch_gemv_t<WT, XT, 2, 4, PRO>(L, a);
}

// Would this launch's grid fit the ArgMax candidate buffer (GemvArgs::amax)?  A tuned grid (fl_tune "gemv_blocks") or a
// device with >= 512 CUs may not: the caller then leaves amax null and token selection scans the logits instead.
bool gemv_leaves_candidates(int dtype, const GemvArgs &a) {
    int R = tune(TK_GEMV_R);
    if (R != 4) R = 2;                                       // (the instantiations launch_gemv_ru picks from)
    return tuned_geometry(a.N, a.K, R, dtype == FL_DTYPE_BF16 ? 2 : 4).blocks + 1 <= kMaxArgmaxCand;
}

int64_t gemv_owner_chunk(int dtype, int64_t N, int64_t K) {
    int R = tune(TK_GEMV_R);
    if (R != 4) R = 2;
    const size_t es = dtype == FL_DTYPE_BF16 ? 2 : 4;
    const int waves = std::max(4, tuned_geometry(N, K, R, es).waves);
    return (int64_t)waves * R * K * (int64_t)es;
}

bool gemv_resid_edge_fits(int dtype, bool one_shard, bool compute_weights, int64_t N, int64_t K, int64_t Nc) {
    GemvResidEdge e;
    e.N = N; e.K = K; e.Nc = Nc; e.cus = device_cu_count();
    e.bf16 = dtype == FL_DTYPE_BF16; e.one_shard = one_shard; e.compute_weights = compute_weights;
    e.force_blocks = g_force_blocks.load(); e.force_waves = g_force_waves.load();
    // (R = 2 whatever "gemv_u" says: launch_gemv_ru; a forced "gemv_r" keeps the norm prologue)
    return tune(TK_GEMV_R) == 2 && gemv_supported(dtype, N, K) && gemv_supported(dtype, Nc, N) && gemv_resid_edge(e);
}

int launch_gemv(Launcher &L, int dtype, const GemvArgs &a) {
    if (a.N <= 0 || a.K <= 0) FL_FAIL(FL_ERR_BAD_ARGUMENT, "launch_gemv: bad shape");
    if (!gemv_supported(dtype, a.N, a.K)) FL_FAIL(FL_ERR_UNSUPPORTED, "launch_gemv: K=%d unsupported", a.K);
    if (a.pro == PRO_NORM && !gemv_norm_supported(dtype, a.N, a.K)) FL_FAIL(FL_ERR_UNSUPPORTED, "fused norm needs K <= 6144");
    if (a.epi == EPI_GATEUP && a.N % 32) FL_FAIL(FL_ERR_BAD_ARGUMENT, "gate/up matrix rows must be a multiple of 32");
    if (a.ll && (a.epi != EPI_F32 || a.bias || a.ll_slot <= 0)) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fused all-reduce: plain fp32 epilogue without bias only");
    if (a.epi == EPI_QKV_ROPE && (a.d <= 0 || a.d % 2 || a.N != (a.H + 2 * a.Hkv) * a.d)) FL_FAIL(FL_ERR_BAD_ARGUMENT, "bad qkv shape");
    if (a.pro != PRO_X && a.pro != PRO_NORM && a.pro != PRO_XS) FL_FAIL(FL_ERR_BAD_ARGUMENT, "launch_gemv: prologue %d", a.pro);
    if (a.epi == EPI_RESID) {
        if (dtype != FL_DTYPE_BF16 || a.pro != PRO_X) FL_FAIL(FL_ERR_UNSUPPORTED, "launch_gemv: the residual epilogue is a bf16 launch with the plain prologue");
        if (a.ll || a.bias || a.x_scale || a.amax) FL_FAIL(FL_ERR_BAD_ARGUMENT, "launch_gemv: the residual epilogue takes no bias, row scale, all-reduce or ArgMax");
        if (!a.x_in || !a.norm_w || !a.x_out || !a.xs_out || !a.cs_out || a.x_in == a.x_out) FL_FAIL(FL_ERR_BAD_ARGUMENT, "launch_gemv: the residual epilogue needs x_in, norm_w, x_out (not x_in), xs_out and cs_out");
        if (a.N % 8) FL_FAIL(FL_ERR_UNSUPPORTED, "launch_gemv: the residual epilogue needs N a multiple of 8");
    }
    if (a.pro == PRO_XS) {
        if (dtype != FL_DTYPE_BF16 || a.ll || a.epi == EPI_RESID) FL_FAIL(FL_ERR_UNSUPPORTED, "launch_gemv: the staged-vector prologue is a bf16 launch with the fp32, gate/up or RoPE epilogue");
        if (!a.x || !a.cs) FL_FAIL(FL_ERR_BAD_ARGUMENT, "launch_gemv: the staged-vector prologue needs x and cs");
        return launch_gemv_ru<bf16_t, bf16_t, PRO_XS>(L, a);
    }
    if (dtype == FL_DTYPE_BF16)
        return a.pro == PRO_NORM ? launch_gemv_ru<bf16_t, bf16_t, PRO_NORM>(L, a) : launch_gemv_ru<bf16_t, bf16_t, PRO_X>(L, a);
    return a.pro == PRO_NORM ? launch_gemv_ru<float, float, PRO_NORM>(L, a) : launch_gemv_ru<float, float, PRO_X>(L, a);
}

}  // namespace fl
