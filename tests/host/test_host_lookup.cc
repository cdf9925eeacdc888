// Stand-alone driver of the prompt-lookup search (fastllm_amd/csrc/lookup.h) for tests/test_host_lookup.py: built with
// -fsanitize=address,undefined, it reads cases from a text file -- one per line: max_draft ngram_max ngram_min limit n_history id... --
// runs each through fl::lookup_draft into a buffer of exactly `limit` words (so a write past the limit is a heap overflow the
// sanitizer reports) and prints "n_draft id..." per case.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "lookup.h"

int main(int argc, char **argv) {
    if (argc != 2) { fprintf(stderr, "usage: %s cases.txt\n", argv[0]); return 2; }
    FILE *f = fopen(argv[1], "r");
    if (!f) { perror(argv[1]); return 2; }
    long n_cases = 0;
    int max_draft, ngram_max, ngram_min;
    unsigned long limit, n;
    while (fscanf(f, "%d %d %d %lu %lu", &max_draft, &ngram_max, &ngram_min, &limit, &n) == 5) {
        std::vector<uint32_t> h(n);
        for (unsigned long i = 0; i < n; i++) {
            unsigned v;
            if (fscanf(f, "%u", &v) != 1) { fprintf(stderr, "case %ld: short history\n", n_cases); return 2; }
            h[i] = v;
        }
        // exactly-sized heap blocks: a read before / past the history or a write past `limit` trips the sanitizer
        uint32_t *hist = n ? (uint32_t *)malloc(n * sizeof(uint32_t)) : nullptr;
        for (unsigned long i = 0; i < n; i++) hist[i] = h[i];
        uint32_t *out = limit ? (uint32_t *)malloc(limit * sizeof(uint32_t)) : nullptr;
        const size_t k = fl::lookup_draft(hist, n, max_draft, ngram_max, ngram_min, limit, out);
        printf("%zu", k);
        for (size_t i = 0; i < k; i++) printf(" %u", out[i]);
        printf("\n");
        free(hist);
        free(out);
        n_cases++;
    }
    fclose(f);
    printf("host lookup driver done %ld\n", n_cases);
    return 0;
}
