// k_logit_rules.hip -- logit bias and repetition / frequency / presence penalties (fl_cache_set_logit_rules): one launch between
// lm_head and token selection inside the captured decode step.
//
// Per vocabulary id the cache keeps {word, bias}: word bit 31 = "occurred in the prompt", bits 0..30 = c, the times the id was
// produced as output.  For the raw fp32 row x the selection sees y, every operation rounded on its own (no FMA), so that a numpy
// float32 restatement reproduces the bits:
//     y = x[j]
//     if word != 0 and rp != 1:  y = y > 0 ? y / rp : y * rp
//     if c > 0:                  y = y - (float)c * fp;  y = y - pp
//     y = y + bias
// The thread that owns element j == the step's input token first adds 1 to its own word (count_input) and stores it back: no
// atomics, no second pass.  Traffic: V x (4 + 8 + 4) bytes per row, mostly from L2.
//
// A thread takes four consecutive ids: one 16-byte load of the row, two of the table, one 16-byte store -- where the row starts on a
// 16-byte boundary in both buffers; rows b > 0 of an odd vocabulary do not, and the last V % 4 ids never fill a vector: those go one
// id at a time.  256 lanes x 4 ids per workgroup: 32 workgroups at V = 32 000, 149 at V = 152 064, capped at 2048 with a grid stride.
#include <algorithm>

#include "kernels.h"
#include "logit_rules_dev.h"                                          // logit_rule, logit_rule_count

namespace fl {

constexpr int kRulesBlock = 256, kRulesPerThread = 4, kRulesMaxGrid = 2048;

__global__ __launch_bounds__(kRulesBlock) void logit_rules_kernel(const float *__restrict__ logits, int V, LogitRulesSrc src) {
    const int b = blockIdx.y;
    const float *__restrict__ x = logits + (size_t)b * V;
    const LogitRulesCtl *ctl = src.ctls ? src.ctls[b] : src.ctl;
    float *__restrict__ y = src.out ? src.out + (size_t)b * V : ctl->out;
    const bool vec = ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y)) & 15) == 0;
    const int nchunk = (V + kRulesPerThread - 1) / kRulesPerThread;
    const int stride = gridDim.x * kRulesBlock;
    if (!ctl) {                                                       // a batch member without rules: its row goes through bit for bit
        for (int c = blockIdx.x * kRulesBlock + threadIdx.x; c < nchunk; c += stride) {
            const int j0 = c * kRulesPerThread;
            if (vec && j0 + kRulesPerThread <= V) {
                *reinterpret_cast<uint4v *>(y + j0) = *reinterpret_cast<const uint4v *>(x + j0);
            } else {
                for (int j = j0; j < min(j0 + kRulesPerThread, V); j++) y[j] = x[j];
            }
        }
        return;
    }
    const float rp = ctl->rp, fp = ctl->fp, pp = ctl->pp;
    LogitRuleEntry *tab = ctl->table;
    const bool vec4 = vec && (reinterpret_cast<uintptr_t>(tab) & 15) == 0;
    const uint32_t token = src.tokens ? src.tokens[b] : (src.seqs ? src.seqs[b].st->token : src.st->token);
    const bool count = ctl->count_input != 0;
    for (int c = blockIdx.x * kRulesBlock + threadIdx.x; c < nchunk; c += stride) {
        const int j0 = c * kRulesPerThread;
        if (vec4 && j0 + kRulesPerThread <= V) {
            const float4v xv = *reinterpret_cast<const float4v *>(x + j0);
            const uint4v t0 = *reinterpret_cast<const uint4v *>(tab + j0);         // {word, bias} of ids j0, j0 + 1
            const uint4v t1 = *reinterpret_cast<const uint4v *>(tab + j0 + 2);     // ... of j0 + 2, j0 + 3
            uint32_t w[4] = {t0[0], t0[2], t1[0], t1[2]};
            const float bs[4] = {__uint_as_float(t0[1]), __uint_as_float(t0[3]), __uint_as_float(t1[1]), __uint_as_float(t1[3])};
            float4v yv;
#pragma unroll
            for (int u = 0; u < 4; u++) {
                if (count && (uint32_t)(j0 + u) == token) { w[u] = logit_rule_count(w[u]); tab[j0 + u].word = w[u]; }
                yv[u] = logit_rule(xv[u], w[u], bs[u], rp, fp, pp);
            }
            *reinterpret_cast<float4v *>(y + j0) = yv;
        } else {
            for (int j = j0; j < min(j0 + kRulesPerThread, V); j++) {
                LogitRuleEntry e = tab[j];
                if (count && (uint32_t)j == token) { e.word = logit_rule_count(e.word); tab[j].word = e.word; }
                y[j] = logit_rule(x[j], e.word, e.bias, rp, fp, pp);
            }
        }
    }
}

int launch_logit_rules(Launcher &L, const float *logits, int64_t V, int rows, const LogitRulesSrc &src) {
    if (rows < 1 || rows > 65535 || V <= 0 || V > 0x7fffffff - kRulesPerThread) FL_FAIL(FL_ERR_BAD_ARGUMENT, "logit_rules: bad shape");
    const int64_t per_wg = (int64_t)kRulesBlock * kRulesPerThread;
    const unsigned gx = (unsigned)std::min<int64_t>((V + per_wg - 1) / per_wg, kRulesMaxGrid);
    const char *tag = L.tag;
    L.tag = "rules";                                                  // the profile lists it as select_advance[rules]
    const int rc = L.launch(KC_ARGMAX, (double)V * 16 * rows, 0, logit_rules_kernel, dim3(gx, (unsigned)rows), dim3(kRulesBlock), 0, logits, (int)V, src);
    L.tag = tag;
    return rc;
}

// a call's scalars, its count_input flag and the cache's buffers, on the stream ahead of the call's steps
__global__ void set_logit_rules_ctl_kernel(LogitRulesCtl *ctl, LogitRulesCtl value) {
    if (threadIdx.x == 0) *ctl = value;
}
int launch_set_logit_rules_ctl(Launcher &L, LogitRulesCtl *ctl, const LogitRulesCtl &value) {
    const char *tag = L.tag;
    L.tag = "rules_ctl";
    const int rc = L.launch(KC_ARGMAX, 0, 0, set_logit_rules_ctl_kernel, dim3(1), dim3(64), 0, ctl, value);
    L.tag = tag;
    return rc;
}

}  // namespace fl
