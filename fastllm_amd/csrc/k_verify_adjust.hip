// k_verify_adjust.hip -- logit rules and the guide inside a verify step (fl_forward_verify_lp, fl_decode_lookup_lp): one launch between
// lm_head of the step's T <= 16 rows and its selection launch (verify_select / verify_sample, unchanged, read `out` in place of the
// raw rows), and one small launch behind the selection that brings the rules table up to date.
//
// Row i of a verify step stands for decode step i of the plain loop: its input is ids[i] (ids[0] the step's token, ids[i] draft[i-1]),
// and the plain loop counts a step's input before it adjusts the step's row.  So row i must see
//     word_i[j] = the table word of id j, counted (logit_rule_count: saturating, prompt bit untouched) once per r <= i with ids[r] == j
//     sigma_i   = the guide state after drafts 0 .. i-1 (the host walked them: VerifyAdjustArgs::states)
// and out[i][j] = logit_rule(x[i][j], word_i[j], bias[j]) for the ids sigma_i allows (the raw bits without rules), -inf for every
// other id.  logit_rule / logit_rule_count are logit_rules_kernel's own code (logit_rules_dev.h), the search guide_mask_kernel's
// (guide_dev.h): a row comes out with the bits the two one-row launches give for the same word and state.
//
// THE TABLE IS ONLY READ HERE: the ids arrive by value with the launch arguments and every workgroup counts for itself, so there
// are no atomics and no order between rows or workgroups.  How many rows the step keeps is known only after the selection came
// back; rules_count_kernel then adds the kept rows' inputs to the table, one lane, serially (an id that occurs twice is counted
// twice), on the same stream ahead of everything submitted later.
//
// Geometry: grid (id ranges, T).  A workgroup of 256 lanes owns the ids [a, e) of one row, a multiple of 4 wide (512 ids; an even
// share where the grid is capped at 2048).  It first keeps, as a bit mask, the rows r <= i whose id lies in [a, e): almost always
// none, and the plain path runs -- no compare per element.  Then
//   rules only    four consecutive ids per lane: one 16-byte load of x, two of the table, one 16-byte store
//   with a guide  the slice of sigma_i's list inside [a, e) by two cooperative searches; the range of out is filled with -inf by
//                 16-byte stores; after a barrier each allowed id t gets its value from x[t] (and table[t]), the list read coalesced.
//                 x is read once and only where allowed, and there is no intermediate row between rules and mask.
// 16-byte accesses only where the row starts on a 16-byte boundary in every buffer involved: rows i > 0 of an odd vocabulary do not,
// and the last V % 4 ids never fill a vector -- those go one id at a time.  Traffic per row at most V x (4 + 8 + 4) bytes, mostly L2.
#include <algorithm>

#include "kernels.h"
#include "logit_rules_dev.h"
#include "guide_dev.h"

namespace fl {

// word_i[j]: one count per kept row whose id is j (mine: the rows r <= i with an id in this workgroup's range)
__device__ __forceinline__ uint32_t verify_word(uint32_t w, uint32_t j, uint32_t mine, const VerifyAdjustArgs &A) {
#pragma unroll
    for (int r = 0; r < kVerifyMaxRows; r++)
        if (((mine >> r) & 1u) && A.ids[r] == j) w = logit_rule_count(w);
    return w;
}

__global__ __launch_bounds__(kGuideBlock) void verify_adjust_kernel(const float *__restrict__ logits, int V, VerifyAdjustArgs A) {
    const int i = blockIdx.y, tid = threadIdx.x;
    const int per = (int)(((V + gridDim.x - 1) / gridDim.x + 3u) & ~3u);
    const int a = blockIdx.x * per, e = min(a + per, V);
    if (a >= V) return;
    const uint32_t *__restrict__ x = reinterpret_cast<const uint32_t *>(logits) + (size_t)i * V;
    uint32_t *__restrict__ y = reinterpret_cast<uint32_t *>(A.out) + (size_t)i * V;
    const LogitRuleEntry *__restrict__ tab = A.table;
    const float rp = A.rp, fp = A.fp, pp = A.pp;
    uint32_t mine = 0;
    if (tab) {
#pragma unroll
        for (int r = 0; r < kVerifyMaxRows; r++)
            if (r <= i && A.ids[r] >= (uint32_t)a && A.ids[r] < (uint32_t)e) mine |= 1u << r;
    }
    if (!A.row_ptr) {                                                 // rules only (the launcher refuses "neither")
        const bool vec = ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(tab)) & 15) == 0;
        for (int j0 = a + tid * 4; j0 < e; j0 += kGuideBlock * 4) {
            if (vec && j0 + 4 <= e) {
                const float4v xv = *reinterpret_cast<const float4v *>(x + j0);
                const uint4v t0 = *reinterpret_cast<const uint4v *>(tab + j0);         // {word, bias} of ids j0, j0 + 1
                const uint4v t1 = *reinterpret_cast<const uint4v *>(tab + j0 + 2);     // ... of j0 + 2, j0 + 3
                uint32_t w[4] = {t0[0], t0[2], t1[0], t1[2]};
                const float bs[4] = {__uint_as_float(t0[1]), __uint_as_float(t0[3]), __uint_as_float(t1[1]), __uint_as_float(t1[3])};
                float4v yv;
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    if (mine) w[u] = verify_word(w[u], (uint32_t)(j0 + u), mine, A);
                    yv[u] = logit_rule(xv[u], w[u], bs[u], rp, fp, pp);
                }
                *reinterpret_cast<float4v *>(y + j0) = yv;
            } else {
                for (int j = j0; j < min(j0 + 4, e); j++) {
                    const LogitRuleEntry en = tab[j];
                    const uint32_t w = mine ? verify_word(en.word, (uint32_t)j, mine, A) : en.word;
                    y[j] = __float_as_uint(logit_rule(__uint_as_float(x[j]), w, en.bias, rp, fp, pp));
                }
            }
        }
        return;
    }
    const uint32_t sigma = A.states[i];
    const uint64_t r0 = A.row_ptr[sigma];
    const uint32_t n = (uint32_t)(A.row_ptr[sigma + 1] - r0);
    const uint32_t *__restrict__ list = A.tokens + r0;
    const uint32_t lo = guide_lower_bound(list, n, (uint32_t)a), hi = guide_lower_bound(list, n, (uint32_t)e);
    const uint32_t ninf = 0xff800000u;
    const bool vec = (reinterpret_cast<uintptr_t>(y) & 15) == 0;      // (a is a multiple of 4)
    for (int j0 = a + tid * 4; j0 < e; j0 += kGuideBlock * 4) {
        if (vec && j0 + 4 <= e) {
            *reinterpret_cast<uint4v *>(y + j0) = uint4v{ninf, ninf, ninf, ninf};
        } else {
            for (int j = j0; j < min(j0 + 4, e); j++) y[j] = ninf;
        }
    }
    __syncthreads();                                                  // the fill of this range is done before its allowed ids are put back
    for (uint32_t k = lo + tid; k < hi; k += kGuideBlock) {
        const uint32_t t = list[k];                                   // (in [a, e): the two searches)
        uint32_t v = x[t];
        if (tab) {
            const LogitRuleEntry en = tab[t];
            const uint32_t w = mine ? verify_word(en.word, t, mine, A) : en.word;
            v = __float_as_uint(logit_rule(__uint_as_float(v), w, en.bias, rp, fp, pp));
        }
        y[t] = v;
    }
}

int launch_verify_adjust(Launcher &L, const float *logits, int64_t V, int T, const VerifyAdjustArgs &a) {
    if (T < 1 || T > kVerifyMaxRows || V <= 0 || V > 0x7fffffff - 4 * kGuideMaxGrid) FL_FAIL(FL_ERR_BAD_ARGUMENT, "verify_adjust: bad shape");
    if (!logits || !a.out || logits == a.out) FL_FAIL(FL_ERR_BAD_ARGUMENT, "verify_adjust: null or aliased rows");
    if (!a.table && !a.row_ptr) FL_FAIL(FL_ERR_BAD_ARGUMENT, "verify_adjust: neither rules nor a guide");
    if (a.row_ptr && !a.tokens) FL_FAIL(FL_ERR_BAD_ARGUMENT, "verify_adjust: a guide without its token lists");
    const unsigned gx = (unsigned)std::min<int64_t>((V + kGuideIdsPerWg - 1) / kGuideIdsPerWg, kGuideMaxGrid);
    const char *tag = L.tag;
    L.tag = "verify_adjust";
    const int rc = L.launch(KC_ARGMAX, (double)V * 16 * T, 0, verify_adjust_kernel, dim3(gx, (unsigned)T), dim3(kGuideBlock), 0, logits, (int)V, a);
    L.tag = tag;
    return rc;
}

// the kept rows' inputs, one more output each: one lane, in order, so an id that occurs twice is counted twice
__global__ void rules_count_kernel(LogitRuleEntry *__restrict__ tab, int V, RulesCountArgs a) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    for (int r = 0; r < a.n && r < kVerifyMaxRows; r++) {
        const uint32_t id = a.ids[r];
        if (id < (uint32_t)V) tab[id].word = logit_rule_count(tab[id].word);
    }
}

int launch_rules_count(Launcher &L, LogitRuleEntry *table, int64_t V, const RulesCountArgs &a) {
    if (!table || V <= 0 || V > 0x7fffffff || a.n < 0 || a.n > kVerifyMaxRows) FL_FAIL(FL_ERR_BAD_ARGUMENT, "rules_count: bad arguments");
    if (a.n == 0) return FL_OK;
    const char *tag = L.tag;
    L.tag = "rules_count";
    const int rc = L.launch(KC_ARGMAX, 0, 0, rules_count_kernel, dim3(1), dim3(64), 0, table, (int)V, a);
    L.tag = tag;
    return rc;
}

}  // namespace fl
