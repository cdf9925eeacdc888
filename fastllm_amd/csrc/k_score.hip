// k_score.hip -- score_rows_kernel: prompt log-probabilities (fl_forward_score, fl_batch_score, fl_op_score).  Every row of a
// [R][V] fp32 logits block is scored against a token the caller names: its log-prob under the row's own distribution, its rank in the
// order "logit descending, lower index first", and the first top_n of that order.  The arithmetic is token_logprobs_kernel's: both
// kernels instantiate logprobs_row (logprobs_dev.h), this one with the rank.
#include "logprobs_dev.h"

namespace fl {

// One workgroup of 1024 lanes per row.  targets[row] >= V (kScoreNoTarget): the row has no target -- lp a quiet NaN, rank 0, the
// tops as for any row.  A row with NaN or without a finite maximum gets unspecified values; every reported id is < V.
__global__ __launch_bounds__(1024) void score_rows_kernel(const float *__restrict__ logits, int V, const uint32_t *__restrict__ targets,
                                                          int top_n, ScoreRec *__restrict__ recs) {
    __shared__ __attribute__((aligned(16))) LogprobLds S;
    const int row = blockIdx.x;
    ScoreRec *__restrict__ rec = recs + row;
    logprobs_row<true>(S, logits + (size_t)row * V, V, max(0, min(min(top_n, kLogprobsMaxTop), V)), targets[row], &rec->lp.chosen, rec->lp.ids,
                       rec->lp.lps, &rec->rank);
}

int launch_score_rows(Launcher &L, const float *logits, int64_t V, int rows, const uint32_t *targets, int top_n, ScoreRec *recs) {
    if (rows < 1 || V <= 0 || V > 0x7fffffff || top_n < 0 || top_n > kLogprobsMaxTop) FL_FAIL(FL_ERR_BAD_ARGUMENT, "score_rows: bad shape");
    const char *tag = L.tag;
    L.tag = "score";                                                     // (the profile lists it apart from the forward's launches)
    const int rc = L.launch(KC_ARGMAX, (double)V * 8 * rows, 0, score_rows_kernel, dim3((unsigned)rows), dim3(1024), 0, logits, (int)V, targets, top_n, recs);
    L.tag = tag;
    return rc;
}

}  // namespace fl
