// argmax_dev.h -- the ArgMax of one logits row by one workgroup of 1024 lanes: shared by the token selection kernels of k_ops.hip and
// the packed verify step's (k_verify_packed.hip), so that every caller takes ties and NaN the same way.
#pragma once
#include "common.h"

namespace fl {

// a workgroup's (value, index) pairs -> the ArgMax in thread 0 (ties -> the larger index; index < 0 = nothing)
__device__ inline int argmax_reduce(float best, int idx, float *bv, int *bi) {
    const int tid = threadIdx.x;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        float ov = __shfl_xor(best, o, 64); int oi = __shfl_xor(idx, o, 64);
        if (oi >= 0 && (idx < 0 || ov > best || (ov == best && oi > idx))) { best = ov; idx = oi; }
    }
    if ((tid & 63) == 0) { bv[tid >> 6] = best; bi[tid >> 6] = idx; }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < 16; w++) {
            float ov = bv[w]; int oi = bi[w];
            if (oi >= 0 && (idx < 0 || ov > best || (ov == best && oi > idx))) { best = ov; idx = oi; }
        }
    }
    return idx < 0 ? 0 : idx;                           // valid in thread 0
}

// ArgMax (temperature None or < 1e-7, App. A.7): iter().enumerate().max_by(total_cmp) -> on exact ties
// the LAST maximal index wins.
__device__ inline int argmax_last(const float *__restrict__ logits, int V, float *bv, int *bi) {
    const int tid = threadIdx.x;
    float best = -INFINITY; int idx = -1;
    auto take = [&](float v, int ii) { if (idx < 0 || v > best || (v == best && ii > idx)) { best = v; idx = ii; } };
    // 16 bytes per lane, eight loads per round trip, all unconditional (past the end a thread re-reads the last chunk and
    // skips it): V = 32000 is ONE round trip.  (Scalar loads with a one-load-per-iteration remainder loop: eleven.)
    const int nvec = (V % 4 == 0 && (reinterpret_cast<uintptr_t>(logits) & 15) == 0) ? V / 4 : 0;
    for (int c0 = tid; c0 < nvec; c0 += 8 * 1024) {
        float4v v[8];
#pragma unroll
        for (int u = 0; u < 8; u++) v[u] = *reinterpret_cast<const float4v *>(logits + 4 * (size_t)min(c0 + u * 1024, nvec - 1));
#pragma unroll
        for (int u = 0; u < 8; u++) {
            const int c = c0 + u * 1024;
            if (c < nvec) {
#pragma unroll
                for (int j = 0; j < 4; j++) take(v[u][j], 4 * c + j);
            }
        }
    }
    for (int i = 4 * nvec + tid; i < V; i += 1024) take(logits[i], i);      // (a vocabulary that is not a multiple of 4)
    return argmax_reduce(best, idx, bv, bi);
}

}  // namespace fl
