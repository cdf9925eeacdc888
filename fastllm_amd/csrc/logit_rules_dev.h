// logit_rules_dev.h -- the arithmetic of the logit rules (fl_cache_set_logit_rules), shared by logit_rules_kernel (k_logit_rules.hip:
// one row, the table counted in place) and verify_adjust_kernel / rules_count_kernel (k_verify_adjust.hip: the rows of a verify step,
// the table only read).  Device code only, the way logprobs_dev.h serves token_logprobs and score_rows: both kernels run this code, so
// a row of a verify step is adjusted to the bits the one-row step gives for the same word.
//
//     y = x[j]
//     if word != 0 and rp != 1:  y = y > 0 ? y / rp : y * rp
//     if c > 0:                  y = y - (float)c * fp;  y = y - pp          (c = word & 0x7fffffff)
//     y = y + bias
// every operation rounded on its own (no FMA), so that a numpy float32 restatement reproduces the bits.
#pragma once
#include "kernels.h"

namespace fl {

__device__ __forceinline__ float logit_rule(float x, uint32_t word, float bias, float rp, float fp, float pp) {
    float y = x;
    if (word != 0 && rp != 1.0f) y = y > 0.0f ? __fdiv_rn(y, rp) : __fmul_rn(y, rp);
    const uint32_t c = word & ~kRulePromptBit;
    if (c > 0) {
        y = __fsub_rn(y, __fmul_rn(__uint2float_rn(c), fp));
        y = __fsub_rn(y, pp);
    }
    return __fadd_rn(y, bias);
}

// one more output of id j (the count saturates at 2^31 - 1: the prompt bit is never carried into)
__device__ __forceinline__ uint32_t logit_rule_count(uint32_t word) { return (word & ~kRulePromptBit) == ~kRulePromptBit ? word : word + 1; }

}  // namespace fl
