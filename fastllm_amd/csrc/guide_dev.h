// guide_dev.h -- the cooperative search of a guide's token lists, shared by guide_mask_kernel (k_guide.hip) and verify_adjust_kernel
// (k_verify_adjust.hip).  Device code only.  A workgroup of kGuideBlock lanes owns kGuideIdsPerWg consecutive ids of a row (or an
// even share of the row where the grid is capped) and finds the slice of a state's ascending list inside its range with two calls.
#pragma once
#include "kernels.h"

namespace fl {

constexpr int kGuideBlock = 256, kGuideIdsPerWg = 512, kGuideMaxGrid = 2048;

// how many of list[0 .. n) (ascending) are < key: the same value in every thread of the workgroup, which calls it as a whole.
// 256 lanes probe 256 evenly spaced entries per round: 3 rounds at 152 064 entries, instead of 17 dependent probes of a bisection.
__device__ __forceinline__ uint32_t guide_lower_bound(const uint32_t *__restrict__ list, uint32_t n, uint32_t key) {
    uint32_t lo = 0, hi = n;                                          // the answer is in [lo, hi]
    while (hi > lo) {
        const uint32_t chunk = (hi - lo + kGuideBlock - 1) / kGuideBlock;
        const uint32_t begin = lo + threadIdx.x * chunk;              // (< 2^32: at most hi + 256 * chunk)
        const uint32_t end = min(begin + chunk, hi);
        const int below = begin < hi && list[end - 1] < key;          // this lane's whole chunk is below the key
        const uint32_t k = (uint32_t)__syncthreads_count(below);      // (monotone: the first k chunks)
        const uint32_t nlo = min(lo + k * chunk, hi);
        if (nlo == hi) return hi;
        lo = nlo;
        hi = min(nlo + chunk, hi) - 1;                                // chunk k ends with an entry >= key
    }
    return lo;
}

}  // namespace fl
