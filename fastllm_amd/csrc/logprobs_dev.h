// logprobs_dev.h -- the two passes over a logits row behind every reported log-probability: token_logprobs_kernel (k_ops.hip: the
// token a decode step selected) and score_rows_kernel (k_score.hip: a token the caller names, and its rank).  Device code only; each
// file instantiates logprobs_row in its own kernel, the way sampler_dev.h serves select_advance and verify_sample.
//
// lp[i] = (x[i] - m) - log(sum_j exp(x[j] - m)), m = max_j x[j]: the model's own distribution (temperature 1, nothing masked).
// One workgroup of 1024 lanes per row.
//
// The row is read TWICE (from L2: 2 * V * 4 bytes, 1.2 MB at V = 152 064), whatever top_n is:
//   pass 1  the maximum, and every lane's largest KEY.  A key is (order-preserving bits of the logit : ~index), so keys are distinct
//           and their descending order is "logit descending, lower index first".  The 1024 lane maxima are sorted in LDS; tau = the
//           top_n-th of them.  At least top_n elements of the row have a key >= tau (those lane maxima themselves), so the top_n largest
//           keys of the row are all >= tau.  kRank: every lane also counts its keys above the target's; the block-wide sum + 1 is the
//           target's rank in that order.
//   pass 2  sum of expf(x - m), fp64 per lane and across lanes; and every key >= tau is gathered into LDS.  Only lanes whose maximum
//           is >= tau can hold such keys, and there are exactly top_n of them: at most top_n * ceil(V / 1024) keys (2980 at
//           V = 152 064), a few dozen on ordinary rows.  They are sorted; the first top_n are the answer, their logits are in the keys.
// That holds for any placement of the winners (all in one lane's stride, all in one 16-byte chunk, ties of the maximum, a flat row).
// Beyond V = kLpKeys * 1024 / 20 = 419 430 an adversarial row can overflow the gather; such a row (and only such a row) is then
// ranked by one masked maximum pass per rank.
// LDS: 64 KB of keys + 0.4 KB; it shares nothing with select_advance's kSelLds.
#pragma once
#include "kernels.h"

namespace fl {

constexpr int kLpKeys = 8192;
struct LogprobLds {
    unsigned long long keys[kLpKeys];
    unsigned long long wkey[16];
    double wsum[16];
    float wmax[16];
    unsigned wcnt[16];
    unsigned n;
};

__device__ inline unsigned long long logit_key(float v, int i) {
    uint32_t u = __float_as_uint(v == 0.f ? 0.f : v);                   // (-0 and +0 are equal values)
    u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    return ((unsigned long long)u << 32) | (unsigned)~(unsigned)i;
}
__device__ inline float logit_key_value(unsigned long long key) {
    const uint32_t u = (uint32_t)(key >> 32);
    return __uint_as_float((u & 0x80000000u) ? (u & 0x7fffffffu) : ~u);
}

// every element of the row once: 16 bytes per lane, eight loads per round trip, all unconditional, as in argmax_last; scalar loads
// where V % 4 != 0 or the row is not 16-byte aligned (rows 1.. of [T][V] with such a V)
template <typename F>
__device__ inline void for_each_logit(const float *__restrict__ x, int V, F &&take) {
    const int tid = threadIdx.x;
    const int nvec = (V % 4 == 0 && (reinterpret_cast<uintptr_t>(x) & 15) == 0) ? V / 4 : 0;
    for (int c0 = tid; c0 < nvec; c0 += 8 * 1024) {
        float4v v[8];
#pragma unroll
        for (int u = 0; u < 8; u++) v[u] = *reinterpret_cast<const float4v *>(x + 4 * (size_t)min(c0 + u * 1024, nvec - 1));
#pragma unroll
        for (int u = 0; u < 8; u++) {
            const int c = c0 + u * 1024;
            if (c < nvec) {
#pragma unroll
                for (int j = 0; j < 4; j++) take(v[u][j], 4 * c + j);
            }
        }
    }
    for (int i = 4 * nvec + tid; i < V; i += 1024) take(x[i], i);
}

// bitonic sort of np (a power of two) keys in LDS, descending; the keys are written and a barrier passed before the call
__device__ inline void sort_keys_desc(unsigned long long *keys, int np) {
    for (int k = 2; k <= np; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = threadIdx.x; t < np / 2; t += 1024) {
                const int a = ((t & ~(j - 1)) << 1) | (t & (j - 1)), b = a | j;
                const unsigned long long ka = keys[a], kb = keys[b];
                if ((ka < kb) == ((a & k) == 0)) { keys[a] = kb; keys[b] = ka; }
            }
            __syncthreads();
        }
    }
}

__device__ inline unsigned long long block_max_key(unsigned long long k, unsigned long long *wkey) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const unsigned long long other = __shfl_xor(k, o, 64); k = other > k ? other : k; }
    __syncthreads();                                                     // (wkey may still be read from the call before)
    if ((threadIdx.x & 63) == 0) wkey[threadIdx.x >> 6] = k;
    __syncthreads();
    k = wkey[0];
    for (int w = 1; w < 16; w++) k = wkey[w] > k ? wkey[w] : k;
    return k;
}

// One row x[V] by the whole workgroup (every lane calls it; all branches are workgroup-uniform).  tok: the token whose log-prob goes
// to *chosen (a quiet NaN where tok >= V: none); ids / lps: the first top_n (0 .. min(kLogprobsMaxTop, V)) of the order.
// kRank: *rank = 1 + the number of ids whose key is above tok's (0 where tok >= V) -- one load of x[tok] ahead of pass 1, one key
// compare per element in it, one block-wide integer sum.
template <bool kRank>
__device__ inline void logprobs_row(LogprobLds &S, const float *__restrict__ x, int V, int top_n, uint32_t tok, float *__restrict__ chosen,
                                    uint32_t *__restrict__ ids, float *__restrict__ lps, uint32_t *__restrict__ rank) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const bool has_tok = tok < (uint32_t)V;

    // ---- pass 1: the maximum and every lane's largest key
    float mx = -INFINITY;
    unsigned long long best = 0;                                         // (a lane without elements: below every real key, whose low word ~index is never 0)
    unsigned long long tkey = ~0ull;                                     // (no target: nothing is above it)
    unsigned above = 0;
    if (kRank && has_tok) tkey = logit_key(x[tok], (int)tok);
    for_each_logit(x, V, [&](float v, int i) {
        mx = fmaxf(mx, v);
        const unsigned long long k = logit_key(v, i);
        best = k > best ? k : best;
        if (kRank) above += k > tkey ? 1u : 0u;
    });
    mx = wave_max(mx);
    if (kRank) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) above += __shfl_xor(above, o, 64);
    }
    if (lane == 0) { S.wmax[wave] = mx; if (kRank) S.wcnt[wave] = above; }
    S.keys[tid] = best;
    if (tid == 0) S.n = 0;
    __syncthreads();
    mx = S.wmax[0];
    for (int w = 1; w < 16; w++) mx = fmaxf(mx, S.wmax[w]);
    if (kRank && tid == 0) {
        unsigned total_above = 0;
        for (int w = 0; w < 16; w++) total_above += S.wcnt[w];
        *rank = has_tok ? total_above + 1u : 0u;
    }
    unsigned long long tau = ~0ull;                                      // top_n == 0: nothing is gathered
    if (top_n > 0) {
        sort_keys_desc(S.keys, 1024);
        tau = S.keys[top_n - 1];                                         // (0 where fewer than top_n lanes hold an element: everything is gathered, V < 80 then)
        __syncthreads();
    }

    // ---- pass 2: the sum of exp(x - m) in fp64, and the keys >= tau
    double acc = 0.0;
    for_each_logit(x, V, [&](float v, int i) {
        acc += (double)expf(__fsub_rn(v, mx));
        const unsigned long long k = logit_key(v, i);
        if (k >= tau) { const unsigned at = atomicAdd(&S.n, 1u); if (at < (unsigned)kLpKeys) S.keys[at] = k; }
    });
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    if (lane == 0) S.wsum[wave] = acc;
    __syncthreads();
    double total = S.wsum[0];
    for (int w = 1; w < 16; w++) total += S.wsum[w];
    const float lz = (float)log(total);
    if (tid == 0) *chosen = has_tok ? __fsub_rn(__fsub_rn(x[tok], mx), lz) : __uint_as_float(0x7fc00000u);
    if (top_n == 0) return;

    const unsigned n = S.n;
    if (n <= (unsigned)kLpKeys) {
        int np = 1;
        while (np < (int)n) np <<= 1;
        for (int j = (int)n + tid; j < np; j += 1024) S.keys[j] = 0;
        __syncthreads();
        sort_keys_desc(S.keys, np);
        if (tid < top_n) {
            const unsigned long long k = S.keys[tid];
            ids[tid] = min(~(uint32_t)k, (uint32_t)(V - 1));             // (n >= top_n real keys; the clamp is for rows with NaN, whose result is unspecified)
            lps[tid] = __fsub_rn(__fsub_rn(logit_key_value(k), mx), lz);
        }
        return;
    }
    // ---- more keys >= tau than the LDS block holds (V > 419 430 and an adversarial row): one masked maximum per rank
    unsigned long long prev = ~0ull;
    for (int r = 0; r < top_n; r++) {
        unsigned long long b = 0;
        for_each_logit(x, V, [&](float v, int i) {
            const unsigned long long k = logit_key(v, i);
            if (k < prev && k > b) b = k;
        });
        b = block_max_key(b, S.wkey);
        if (tid == 0) {
            ids[r] = min(~(uint32_t)b, (uint32_t)(V - 1));
            lps[r] = __fsub_rn(__fsub_rn(logit_key_value(b), mx), lz);
        }
        prev = b;
    }
}

}  // namespace fl
