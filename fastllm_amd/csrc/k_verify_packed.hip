// k_verify_packed.hip -- the selection launch of a PACKED verify step (fl_batch_verify): the rows of several members' verify steps
// back to back in one forward, each row selected as its member's single step selects it -- argmax_last (argmax_dev.h) or sample_all
// (sampler_dev.h), both unchanged -- and one acceptance scan per member.  A file of its own for the reason k_verify_sample.hip is.
#include "argmax_dev.h"
#include "kernels.h"
#include "sampler_dev.h"

namespace fl {

// logits: [R][V], rows r0 .. r0 + R of a pack of T_total rows (one lm_head block); one workgroup of 1024 lanes per row.  Row r is
// token a.rows[r].t of member s = a.rows[r].seq, whose rows are seq_off[s] .. seq_off[s] + seq_cnt[s] and whose ids there are
// [token, draft ..].  The member's SampleState decides the row's selection (the branch is uniform per workgroup; one launch may mix):
//   on == 0: argmax_last -- ties take the last maximal index, NaN as in select_advance;
//   else:    sample_all on an LDS copy of the state whose 64-bit word index is advanced by t, the carry into the high word taken as
//            verify_sample_kernel takes it; kept (or null): [T_total], what top_filter kept for the row (V without a filter and for
//            ArgMax rows); scratch: [R][V] floats, row r's probabilities at (r - r0) * V.
// Acceptance, nobody waits for anybody: lane 0 publishes the row's id, fences and takes a ticket from the member's ticket word; the
// workgroup that draws seq_cnt[s] - 1 scans the member's ids -- n_acc[s] = the largest j <= seq_cnt[s] - 1 with
// ids[seq_off[s] + 1 + k] == out[seq_off[s] + k] for all k < j -- stores it and puts the ticket back to 0.  The tickets live in global
// memory, so a member whose rows straddle two blocks is completed by whichever launch brings its last row (the launches of one pack
// are stream-ordered).  out: kVerifyPackedWords words, zero before the FIRST launch and never memset again.
__global__ __launch_bounds__(1024) void verify_packed_kernel(const float *__restrict__ logits, int V, int r0, const VerifyPackedArgs a,
                                                             float *__restrict__ scratch) {
    __shared__ __attribute__((aligned(16))) unsigned char lds[kSelLds];
    __shared__ float bv[16], bcast[2];
    __shared__ int bi[16], count;
    __shared__ SampleState mine;
    const int row = r0 + (int)blockIdx.x;
    const PackedRow pr = a.rows[row];
    const SampleState *ss = reinterpret_cast<const SampleState *>(reinterpret_cast<const char *>(a.ss) + (size_t)pr.seq * a.ss_stride);
    const bool sampled = __builtin_amdgcn_readfirstlane((int)ss->on) != 0;
    const float *mine_row = logits + (size_t)blockIdx.x * V;
    int idx;
    if (sampled) {
        if (threadIdx.x == 0) {
            mine = *ss;
            const uint64_t w = (((uint64_t)ss->draw_hi << 32) | ss->draw_lo) + (uint64_t)pr.t;
            mine.draw_lo = (uint32_t)w; mine.draw_hi = (uint32_t)(w >> 32);
            mine.kept = (uint32_t)V;
        }
        __syncthreads();
        idx = sample_all(mine_row, V, &mine, scratch + (size_t)blockIdx.x * V, bv, lds, bcast, &count);
    } else {
        idx = argmax_last(mine_row, V, bv, bi);
    }
    if (threadIdx.x != 0) return;
    if (a.kept) a.kept[row] = sampled ? mine.kept : (uint32_t)V;
    uint32_t *out = a.out;
    __hip_atomic_store(&out[row], (uint32_t)idx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __threadfence();                                                   // the id is visible before the ticket is
    const int first = a.seq_off[pr.seq], cnt = a.seq_cnt[pr.seq];
    uint32_t *ticket_word = &out[kVerifyPackedTicket + pr.seq];
    const uint32_t ticket = __hip_atomic_fetch_add(ticket_word, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
    if (ticket != (uint32_t)(cnt - 1)) return;
    __threadfence();
    uint32_t n = 0;
    while (n < (uint32_t)(cnt - 1) && a.ids[first + 1 + n] == __hip_atomic_load(&out[first + n], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) n++;
    out[kVerifyPackedNacc + pr.seq] = n;
    __hip_atomic_store(ticket_word, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

int launch_verify_packed(Launcher &L, const float *logits, int64_t V, int r0, int R, int T_total, const VerifyPackedArgs &a, float *scratch,
                         bool any_sampled) {
    if (T_total < 1 || T_total > kVerifyPackedMaxRows || r0 < 0 || R < 1 || r0 + R > T_total || V <= 0 || V > 0x7fffffff)
        FL_FAIL(FL_ERR_BAD_ARGUMENT, "verify_packed: bad shape");
    if (!logits || !a.rows || !a.seq_off || !a.seq_cnt || !a.ss || !a.ids || !a.out || a.ss_stride < sizeof(SampleState) || (any_sampled && !scratch))
        FL_FAIL(FL_ERR_BAD_ARGUMENT, "verify_packed: null argument");
    return L.launch(KC_ARGMAX, (double)V * 4 * (any_sampled ? 3 : 1) * R, 0, verify_packed_kernel, dim3((unsigned)R), dim3(1024), 0, logits, (int)V,
                    r0, a, scratch);
}

}  // namespace fl
