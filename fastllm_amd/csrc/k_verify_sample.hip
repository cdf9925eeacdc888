// k_verify_sample.hip -- the selection launch of a SAMPLED verify step (fl_forward_verify_ex): one draw per row with the row's own
// word of the seeded stream, then verify_select's acceptance scan.  A file of its own so that sample_all has here its one caller and
// in k_ops.hip the callers it always had: each file inlines it as before.
#include "sampler_dev.h"

namespace fl {

// ------------------------------------------------------------------------------- verify step, sampled: one draw per row + the same scan
// fl_forward_verify_ex: row i is drawn as select_advance_kernel draws one row -- sample_all, unchanged -- with word w0 + i of the
// request's ChaCha12 stream (w0: the 64-bit index in ss.draw_lo / draw_hi; the carry into the high word is taken here).  The
// sampler is a pure function of (row, settings, word index), and a prompt-lookup draft is deterministic, so "the draw of row i is
// draft[i]" IS the acceptance event of rejection sampling against that draft: the accepted prefix is the longest one the draws
// confirm, and every emitted token is the one the one-row loop draws with the same word.  Lane 0 of a workgroup writes the row's
// own SampleState into LDS and sample_all runs on that copy (the word it advances there is dropped: the host is authoritative for
// the draw count, as it is for the cache length).  scratch: [T][V] floats (a row's probabilities / cumulative weights); kept (or
// null): [T], what top_filter kept for the row (V without a filter).  out and the arrival ticket: verify_select_kernel's.
__global__ __launch_bounds__(1024) void verify_sample_kernel(const float *__restrict__ logits, int V, int T,
                                                             const uint32_t *__restrict__ draft, const SampleState ss0,
                                                             float *__restrict__ scratch, uint32_t *__restrict__ out,
                                                             uint32_t *__restrict__ kept) {
    __shared__ __attribute__((aligned(16))) unsigned char lds[kSelLds];
    __shared__ float bv[16], bcast[2];
    __shared__ int count;
    __shared__ SampleState mine;
    const int row = blockIdx.x;
    if (threadIdx.x == 0) {
        mine = ss0;
        const uint64_t w = (((uint64_t)ss0.draw_hi << 32) | ss0.draw_lo) + (uint64_t)row;
        mine.draw_lo = (uint32_t)w; mine.draw_hi = (uint32_t)(w >> 32);
        mine.kept = (uint32_t)V;
    }
    __syncthreads();
    const int idx = sample_all(logits + (size_t)row * V, V, &mine, scratch + (size_t)row * V, bv, lds, bcast, &count);
    if (threadIdx.x != 0) return;
    if (kept) kept[row] = mine.kept;
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

int launch_verify_sample(Launcher &L, const float *logits, int64_t V, int T, const uint32_t *draft, const SampleState &ss, float *scratch,
                         uint32_t *out, uint32_t *kept) {
    if (T < 1 || T > kVerifyMaxRows || V <= 0 || V > 0x7fffffff) FL_FAIL(FL_ERR_BAD_ARGUMENT, "verify_sample: bad shape");
    if (!ss.on) FL_FAIL(FL_ERR_BAD_ARGUMENT, "verify_sample: ArgMax (temperature below 1e-7) is verify_select's");
    return L.launch(KC_ARGMAX, (double)V * 4 * 3 * T, 0, verify_sample_kernel, dim3((unsigned)T), dim3(1024), 0, logits, (int)V, T, draft, ss,
                    scratch, out, kept);
}

}  // namespace fl
