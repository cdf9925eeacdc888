// k_guide.hip -- guided decoding (fl_cache_set_guide): a token-level finite automaton applied inside the captured decode step, one
// launch between lm_head (or the logit-rules launch) and token selection.
//
// The automaton is CSR: state s allows tokens[row_ptr[s] .. row_ptr[s + 1]) (ascending) and tokens[e] leads to next[e].  For the row x
// the selection would have read, it reads y instead: y[j] = x[j] bit for bit where j is in the current state's list, -inf elsewhere.
// fl_guide_create has validated the arrays -- row_ptr starts at 0 and does not decrease, every state has an edge, every list is strictly
// ascending with ids < V, every next < n_states -- and the install the state, so the kernel indexes them WITHOUT further checks.
//
// The advance is in the same launch (no second one): at a step with StepState.step > 0 every workgroup first looks up the edge of the
// step's input token (the previous step's output) in the previous state's list; step 0 of a chunk starts from the state the host
// wrote.  Workgroups of one launch must not read a word another one writes, so there are two state words indexed by step parity: all
// read state[step & 1], workgroup 0 alone writes state[(step + 1) & 1].  A token without an edge leaves the state where it is.
//
// A workgroup owns a contiguous id range [a, e), a multiple of 4 wide.  It finds the slice of the state's list inside its range with
// two cooperative searches (256 lanes probe 256 evenly spaced entries per round: 3 rounds at 152 064 entries, instead of 17 dependent
// probes of a bisection), writes its range of y as -inf -- 16-byte stores where the row starts on a 16-byte boundary; rows b > 0 of an
// odd vocabulary do not, and the last V % 4 ids never fill a vector -- and after a barrier copies x[tok] to y[tok] for the slice, the
// list read coalesced.  x and y are always different buffers (with rules installed x is the rule-adjusted row).  Traffic per row:
// V x 4 bytes written + 4 bytes per allowed id from each of tokens and x.  297 workgroups at V = 152 064, capped at 2048.
#include <algorithm>

#include "kernels.h"
#include "guide_dev.h"                                                // kGuideBlock .., guide_lower_bound

namespace fl {

__global__ __launch_bounds__(kGuideBlock) void guide_mask_kernel(const float *__restrict__ logits, int V, GuideSrc src) {
    const int b = blockIdx.y, tid = threadIdx.x;
    const int per = (int)(((V + gridDim.x - 1) / gridDim.x + 3u) & ~3u);
    const int a = blockIdx.x * per, e = min(a + per, V);
    if (a >= V) return;
    const uint32_t *__restrict__ x = reinterpret_cast<const uint32_t *>(logits) + (size_t)b * V;
    GuideCtl *ctl = src.ctls ? src.ctls[b] : src.ctl;
    uint32_t *__restrict__ y = reinterpret_cast<uint32_t *>(src.out ? src.out + (size_t)b * V : ctl->out);
    if (!ctl) {                                                       // a batch member without a guide: its row goes through bit for bit
        const bool vec = ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y)) & 15) == 0;
        for (int j0 = a + tid * 4; j0 < e; j0 += kGuideBlock * 4) {
            if (vec && j0 + 4 <= e) {
                *reinterpret_cast<uint4v *>(y + j0) = *reinterpret_cast<const uint4v *>(x + j0);
            } else {
                for (int j = j0; j < min(j0 + 4, e); j++) y[j] = x[j];
            }
        }
        return;
    }
    const StepState *st = src.seqs ? src.seqs[b].st : src.st;
    const uint32_t step = st ? st->step : 1u;                         // (the op entry point: always an advance, from state[1])
    const uint64_t *__restrict__ rp = ctl->row_ptr;
    uint32_t sigma = ctl->state[step & 1];
    uint64_t r0 = rp[sigma];
    uint32_t n = (uint32_t)(rp[sigma + 1] - r0);
    if (step > 0) {
        const uint32_t tok = src.tokens ? src.tokens[b] : st->token;
        const uint32_t i = guide_lower_bound(ctl->tokens + r0, n, tok);
        if (i < n && ctl->tokens[r0 + i] == tok) {
            sigma = ctl->next[r0 + i];
            r0 = rp[sigma];
            n = (uint32_t)(rp[sigma + 1] - r0);
        }
    }
    if (blockIdx.x == 0 && tid == 0) ctl->state[(step + 1) & 1] = sigma;
    const uint32_t *__restrict__ list = ctl->tokens + r0;
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
    for (uint32_t i = lo + tid; i < hi; i += kGuideBlock) {
        const uint32_t t = list[i];
        y[t] = x[t];
    }
}

int launch_guide_mask(Launcher &L, const float *logits, int64_t V, int rows, const GuideSrc &src) {
    if (rows < 1 || rows > 65535 || V <= 0 || V > 0x7fffffff - 4 * kGuideMaxGrid) FL_FAIL(FL_ERR_BAD_ARGUMENT, "guide_mask: bad shape");
    const unsigned gx = (unsigned)std::min<int64_t>((V + kGuideIdsPerWg - 1) / kGuideIdsPerWg, kGuideMaxGrid);
    const char *tag = L.tag;
    L.tag = "guide";                                                  // the profile lists it as select_advance[guide]
    const int rc = L.launch(KC_ARGMAX, (double)V * 8 * rows, 0, guide_mask_kernel, dim3(gx, (unsigned)rows), dim3(kGuideBlock), 0, logits, (int)V, src);
    L.tag = tag;
    return rc;
}

// the cache's guide arrays, its output row and the state the host holds, on the stream ahead of a call's (or chunk's) steps
__global__ void set_guide_ctl_kernel(GuideCtl *ctl, GuideCtl value) {
    if (threadIdx.x == 0) *ctl = value;
}
int launch_set_guide_ctl(Launcher &L, GuideCtl *ctl, const GuideCtl &value) {
    const char *tag = L.tag;
    L.tag = "guide_ctl";
    const int rc = L.launch(KC_ARGMAX, 0, 0, set_guide_ctl_kernel, dim3(1), dim3(64), 0, ctl, value);
    L.tag = tag;
    return rc;
}

}  // namespace fl
