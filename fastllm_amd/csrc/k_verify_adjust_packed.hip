// k_verify_adjust_packed.hip -- logit rules and the guide inside a PACKED verify step (fl_batch_verify_lp, fl_batch_decode_lookup_lp):
// one launch per lm_head block between the block's lm_head and its launch_verify_packed (which then reads `out` in place of the raw
// rows), and one small launch behind the LAST block's selection that brings every ruled member's table up to date.
//
// The pack is the one of k_verify_packed.hip: T_total <= 1024 rows, member s = rows seq_off[s] .. seq_off[s] + seq_cnt[s] (1..16 of
// them), its input ids in the pack's id table.  What differs per member travels in a device array of VerifyAdjustMember (kernels.h),
// uploaded with the pack's table image: the rules table or null, the three scalars, the guide's CSR arrays or null, the <= 16 guide
// states the host walked, the member's EOS for the count launch.  Row t of member s comes out exactly as verify_adjust_kernel
// (k_verify_adjust.hip) writes row t of a single step -- the same logit_rules_dev.h / guide_dev.h code:
//     word_t[j] = s's table word of id j, counted once per row r <= t OF THE SAME MEMBER with ids[r] == j
//     out[t][j] = logit_rule(x[t][j], word_t[j], bias[j]) where s's guide state t allows j (the raw bits without rules), -inf elsewhere
// and a member with neither rules nor a guide has its rows copied through bit for bit, so a pack may mix all four kinds.
//
// THE TABLES ARE ONLY READ by the adjust launch: no atomics, no order between rows, members or workgroups.  A member whose rows
// straddle two lm_head blocks needs nothing special: the ids of its earlier rows are read from the pack's id table, not from the
// block, and the later launch counts them again for itself.
//
// Work split: grid (id ranges, members with a row in the block).  A workgroup of 256 lanes owns ONE id range of ONE member for ALL of
// that member's rows in the block, and walks the range in chunks of 1024 ids -- four consecutive ids per lane.  Per chunk
//   * the rows r of the member whose id lies in the chunk are found once, as a bit mask -- almost always empty, and then no row
//     costs a compare per element;
//   * the four table entries of a lane are loaded once, by two 16-byte loads, and stay in eight registers while the member's rows
//     go by.  Rows are walked in ascending t, so "counted once per r <= t" is incremental: at row t the one lane that owns ids[t]
//     counts its register, and the registers are word_t for the row.  Table traffic is 8 V bytes per member and block, not per row;
//   * rules only: per row one 16-byte load of x, the arithmetic on registers, one 16-byte store;
//   * with a guide: the registers are also kept in 8 KB of LDS (rewritten only at the first row and behind a row whose id lies in the
//     chunk), because the ids a state allows are not the ids a lane owns.  Each row has its own cooperative search of its state's
//     list for the chunk's slice (two guide_lower_bound calls), the chunk of out is filled with -inf by 16-byte stores, and behind
//     a barrier every allowed id gets its value from x (read only there) and the LDS entry.  No intermediate row between rules and
//     mask, and the mask is last.
// 16-byte accesses to x / out only where the row starts on a 16-byte boundary in both (rows of an odd V mostly do not), to the table
// only where it does; a lane whose four ids do not all lie below the range's end -- the last V % 4 ids -- goes one id at a time.
//
// Width and grid cap.  1024 ids per chunk is what 256 lanes hold in registers at four ids each, and four is what one 16-byte access
// of x moves.  The range of a workgroup is one chunk up to V = 262 144 (grid.x <= 256): at V = 152 064 that is 149 ranges, and a block
// of 1024 rows with 64 members of 16 gives 149 x 64 = 9536 workgroups of 16 rows x 4 KB each -- 37 per CU on 256 CUs, enough to hide
// the tail, with 64 KB moved per workgroup against one table read of 8 KB.  A narrower chunk (two ids per lane) halves the bytes per
// access; a wider one (eight) doubles the registers for no fewer table bytes.  Beyond 262 144 ids the ranges grow by whole chunks, so
// the grid never exceeds 256 x 64 = 16 384 workgroups whatever V is.  grid.y is the number of members that have a row in the block,
// known to the host from the offsets, so no workgroup is launched for a member outside it (the kernel still checks).
#include <algorithm>

#include "kernels.h"
#include "logit_rules_dev.h"
#include "guide_dev.h"

namespace fl {

constexpr int kVapChunk = kGuideBlock * 4, kVapMaxGridX = 256;

__global__ __launch_bounds__(kGuideBlock) void verify_adjust_packed_kernel(const float *__restrict__ logits, int V, int r0, int R, int n_seq,
                                                                            VerifyAdjustPackedArgs A) {
    __shared__ uint32_t s_word[kVapChunk];
    __shared__ float s_bias[kVapChunk];
    const int tid = threadIdx.x;
    const int s = A.rows[r0].seq + (int)blockIdx.y;
    if (s >= n_seq) return;
    const int off = A.seq_off[s], cnt = min(A.seq_cnt[s], kVerifyMaxRows);
    const int t_lo = max(0, r0 - off), t_hi = min(cnt, r0 + R - off);    // the member's rows in this block
    if (t_lo >= t_hi) return;
    const int per = (int)(((V + gridDim.x - 1) / gridDim.x + kVapChunk - 1) / kVapChunk) * kVapChunk;
    const int a = blockIdx.x * per, e = min(a + per, V);
    if (a >= V) return;
    const VerifyAdjustMember *__restrict__ M = A.members + s;
    const LogitRuleEntry *__restrict__ tab = M->table;
    const uint64_t *__restrict__ row_ptr = M->row_ptr;
    const uint32_t *__restrict__ gtok = M->tokens;
    const float rp = M->rp, fp = M->fp, pp = M->pp;
    const uint32_t *__restrict__ mid = A.ids + off;                      // the member's input ids, row 0 first
    const uint32_t *__restrict__ xb = reinterpret_cast<const uint32_t *>(logits);
    uint32_t *__restrict__ yb = reinterpret_cast<uint32_t *>(A.out);
    const bool tab_vec = (reinterpret_cast<uintptr_t>(tab) & 15) == 0;
    const uint32_t ninf = 0xff800000u;

    for (int c0 = a; c0 < e; c0 += kVapChunk) {
        const int ce = min(c0 + kVapChunk, e);
        const int j0 = c0 + tid * 4;                                     // this lane's ids: j0 .. j0 + nv
        const int nv = max(0, min(4, ce - j0));
        uint32_t mine = 0;                                               // the member's rows whose id lies in [c0, ce)
        uint32_t w[4] = {0u, 0u, 0u, 0u};
        float bs[4] = {0.f, 0.f, 0.f, 0.f};
        if (tab) {
#pragma unroll
            for (int r = 0; r < kVerifyMaxRows; r++)
                if (r < t_hi && mid[r] >= (uint32_t)c0 && mid[r] < (uint32_t)ce) mine |= 1u << r;
            if (nv == 4 && tab_vec) {
                const uint4v e0 = *reinterpret_cast<const uint4v *>(tab + j0);         // {word, bias} of ids j0, j0 + 1
                const uint4v e1 = *reinterpret_cast<const uint4v *>(tab + j0 + 2);     // ... of j0 + 2, j0 + 3
                w[0] = e0[0]; w[1] = e0[2]; w[2] = e1[0]; w[3] = e1[2];
                bs[0] = __uint_as_float(e0[1]); bs[1] = __uint_as_float(e0[3]); bs[2] = __uint_as_float(e1[1]); bs[3] = __uint_as_float(e1[3]);
            } else {
#pragma unroll
                for (int u = 0; u < 4; u++)
                    if (u < nv) { const LogitRuleEntry en = tab[j0 + u]; w[u] = en.word; bs[u] = en.bias; }
            }
            if (mine & ((1u << t_lo) - 1u)) {                            // rows of an earlier block: their ids count for every row here
                for (int r = 0; r < t_lo; r++) {
                    if (!((mine >> r) & 1u)) continue;
                    const uint32_t id = mid[r];
#pragma unroll
                    for (int u = 0; u < 4; u++) if (id == (uint32_t)(j0 + u)) w[u] = logit_rule_count(w[u]);
                }
            }
        }
        for (int t = t_lo; t < t_hi; t++) {
            const bool hit = (mine >> t) & 1u;                           // (the same in every lane)
            if (hit) {
                const uint32_t id = mid[t];
#pragma unroll
                for (int u = 0; u < 4; u++) if (id == (uint32_t)(j0 + u)) w[u] = logit_rule_count(w[u]);
            }
            const size_t row = (size_t)(off + t - r0) * (size_t)V;
            const uint32_t *__restrict__ x = xb + row;
            uint32_t *__restrict__ y = yb + row;
            const bool vec = nv == 4 && ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y)) & 15) == 0;
            if (!row_ptr) {                                              // rules only, or neither: the row copied through
                if (vec) {
                    uint4v v = *reinterpret_cast<const uint4v *>(x + j0);
                    if (tab) {
#pragma unroll
                        for (int u = 0; u < 4; u++) v[u] = __float_as_uint(logit_rule(__uint_as_float(v[u]), w[u], bs[u], rp, fp, pp));
                    }
                    *reinterpret_cast<uint4v *>(y + j0) = v;
                } else {
#pragma unroll
                    for (int u = 0; u < 4; u++) {
                        if (u >= nv) continue;
                        const uint32_t v = x[j0 + u];
                        y[j0 + u] = tab ? __float_as_uint(logit_rule(__uint_as_float(v), w[u], bs[u], rp, fp, pp)) : v;
                    }
                }
                continue;
            }
            if (tab && (t == t_lo || hit)) {
                __syncthreads();                                         // the row before has read the entries it needed
#pragma unroll
                for (int u = 0; u < 4; u++)
                    if (u < nv) { s_word[tid * 4 + u] = w[u]; s_bias[tid * 4 + u] = bs[u]; }
            }
            const uint32_t sigma = M->states[t];
            const uint64_t l0 = row_ptr[sigma];
            const uint32_t n = (uint32_t)(row_ptr[sigma + 1] - l0);
            const uint32_t *__restrict__ list = gtok + l0;
            const uint32_t lo = guide_lower_bound(list, n, (uint32_t)c0), hi = guide_lower_bound(list, n, (uint32_t)ce);
            if (vec) {
                *reinterpret_cast<uint4v *>(y + j0) = uint4v{ninf, ninf, ninf, ninf};
            } else {
#pragma unroll
                for (int u = 0; u < 4; u++) if (u < nv) y[j0 + u] = ninf;
            }
            __syncthreads();                                             // the fill of this chunk (and the LDS entries) before the put-back
            for (uint32_t k = lo + tid; k < hi; k += kGuideBlock) {
                const uint32_t id = list[k];                             // (in [c0, ce): the two searches)
                uint32_t v = x[id];
                if (tab) v = __float_as_uint(logit_rule(__uint_as_float(v), s_word[id - (uint32_t)c0], s_bias[id - (uint32_t)c0], rp, fp, pp));
                y[id] = v;
            }
        }
    }
}

int launch_verify_adjust_packed(Launcher &L, const float *logits, int64_t V, int r0, int R, int T_total, int n_seq, int n_members,
                                const VerifyAdjustPackedArgs &a) {
    if (V <= 0 || V > 0x7fffffff - 2 * kVapChunk * kVapMaxGridX) FL_FAIL(FL_ERR_BAD_ARGUMENT, "verify_adjust_packed: bad vocabulary size");
    if (T_total < 1 || T_total > kVerifyPackedMaxRows || r0 < 0 || R < 1 || r0 + R > T_total)
        FL_FAIL(FL_ERR_BAD_ARGUMENT, "verify_adjust_packed: rows %d .. %d of a pack of %d (at most %d)", r0, r0 + R, T_total, kVerifyPackedMaxRows);
    if (n_seq < 1 || n_seq > kVerifyPackedAux - kVerifyPackedNacc || n_members < 1 || n_members > n_seq || n_members > R)
        FL_FAIL(FL_ERR_BAD_ARGUMENT, "verify_adjust_packed: %d of %d members in a block of %d rows", n_members, n_seq, R);
    if (!logits || !a.out || logits == a.out) FL_FAIL(FL_ERR_BAD_ARGUMENT, "verify_adjust_packed: null or aliased rows");
    if (!a.rows || !a.seq_off || !a.seq_cnt || !a.ids || !a.members) FL_FAIL(FL_ERR_BAD_ARGUMENT, "verify_adjust_packed: a null table");
    const unsigned gx = (unsigned)std::min<int64_t>((V + kVapChunk - 1) / kVapChunk, kVapMaxGridX);
    const char *tag = L.tag;
    L.tag = "verify_adjust_packed";
    const int rc = L.launch(KC_ARGMAX, (double)V * (8.0 * R + 8.0 * n_members), 0, verify_adjust_packed_kernel, dim3(gx, (unsigned)n_members),
                            dim3(kGuideBlock), 0, logits, (int)V, r0, R, n_seq, a);
    L.tag = tag;
    return rc;
}

// Behind the last block's selection: per ruled member ONE lane, serially, so an id that occurs twice is counted twice.  The member
// keeps rows 0 .. n_acc (the selection's accepted count, read from its out block on the device: no host round trip) -- or rows 0 .. k
// where returned id k is the member's EOS (fl_decode_lookup_lp's rule: the plain loop stopped there) -- and their inputs are counted.
__global__ void rules_count_packed_kernel(int V, int n_seq, VerifyAdjustPackedArgs A, const uint32_t *__restrict__ sel) {
    const int s = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (s >= n_seq) return;
    LogitRuleEntry *tab = A.members[s].table;
    if (!tab) return;
    const int off = A.seq_off[s], cnt = min(A.seq_cnt[s], kVerifyMaxRows);
    int n = (int)min(sel[kVerifyPackedNacc + s], (uint32_t)(cnt - 1)) + 1;
    const int64_t eos = A.members[s].eos;
    if (eos >= 0)
        for (int k = 0; k < n; k++)
            if ((int64_t)sel[off + k] == eos) { n = k + 1; break; }
    for (int r = 0; r < n; r++) {
        const uint32_t id = A.ids[off + r];
        if (id < (uint32_t)V) tab[id].word = logit_rule_count(tab[id].word);
    }
}

int launch_rules_count_packed(Launcher &L, int64_t V, int n_seq, const VerifyAdjustPackedArgs &a, const uint32_t *sel_out) {
    if (V <= 0 || V > 0x7fffffff || n_seq < 1 || n_seq > kVerifyPackedAux - kVerifyPackedNacc) FL_FAIL(FL_ERR_BAD_ARGUMENT, "rules_count_packed: bad shape");
    if (!a.seq_off || !a.seq_cnt || !a.ids || !a.members || !sel_out) FL_FAIL(FL_ERR_BAD_ARGUMENT, "rules_count_packed: a null table");
    const char *tag = L.tag;
    L.tag = "rules_count_packed";
    const int rc = L.launch(KC_ARGMAX, 0, 0, rules_count_packed_kernel, dim3((unsigned)((n_seq + 63) / 64)), dim3(64), 0, (int)V, n_seq, a, sel_out);
    L.tag = tag;
    return rc;
}

}  // namespace fl
