// lookup.h -- prompt-lookup drafting (fl_lookup_draft): plain C++, no HIP.  api.hip includes it, and so does the stand-alone host
// test (tests/host/test_host_lookup.cc), so the search exists once.
//
// The rule (include/fastllm_mi355x.h restates it):
//   for n = ngram_max down to ngram_min, with n < n_history: the pattern is the last n ids of `history`; take the largest start s
//   with s + n < n_history and history[s .. s+n) == pattern -- the most recent EARLIER occurrence that has at least one id after
//   it.  The draft is history[s+n ..], cut to min(max_draft, limit) ids and to the end of history.  The first n that matches wins.
#pragma once
#include <cstddef>
#include <cstdint>

namespace fl {

constexpr int kLookupMaxNgram = 8;

// returns the number of ids written to draft_out (<= min(max_draft, limit)); 0: no match
inline size_t lookup_draft(const uint32_t *history, size_t n_history, int max_draft, int ngram_max, int ngram_min, size_t limit,
                           uint32_t *draft_out) {
    size_t want = max_draft > 0 ? (size_t)max_draft : 0;
    if (limit < want) want = limit;
    if (want == 0) return 0;
    for (int n = ngram_max; n >= ngram_min && n >= 1; n--) {
        const size_t nn = (size_t)n;
        if (nn >= n_history) continue;
        const uint32_t *pat = history + (n_history - nn);
        for (size_t s = n_history - nn; s-- > 0;) {                 // s + n < n_history  <=>  s <= n_history - n - 1
            size_t j = 0;
            while (j < nn && history[s + j] == pat[j]) j++;
            if (j < nn) continue;
            const size_t from = s + nn, avail = n_history - from;   // (>= 1)
            const size_t k = avail < want ? avail : want;
            for (size_t i = 0; i < k; i++) draft_out[i] = history[from + i];
            return k;
        }
    }
    return 0;
}

}  // namespace fl
