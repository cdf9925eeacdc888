// Stand-alone driver of the host LogitsProcessor's top-p / top-k path (tests/test_host_top_p.py; built with ASan + UBSan):
//   argv[1]: a file of float32 probabilities; argv[2..6]: top_p (<= 0: none), top_k (0: none), seed, draws to skip, draws
// prints "tok kept" per draw, then "host top-p driver done".
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../fastllm_amd/host/fastllm_host.hpp"

int main(int argc, char **argv) {
    if (argc != 7) { std::fprintf(stderr, "usage: %s prs.f32 top_p top_k seed skip draws\n", argv[0]); return 2; }
    std::FILE *f = std::fopen(argv[1], "rb");
    if (!f) { std::perror(argv[1]); return 2; }
    std::vector<float> prs;
    float buf[4096];
    size_t got;
    while ((got = std::fread(buf, 4, 4096, f)) > 0) prs.insert(prs.end(), buf, buf + got);
    std::fclose(f);
    const double top_p = std::atof(argv[2]);
    const size_t top_k = (size_t)std::strtoull(argv[3], nullptr, 10);
    const uint64_t seed = std::strtoull(argv[4], nullptr, 10);
    const long skip = std::atol(argv[5]), draws = std::atol(argv[6]);
    try {
        fastllm::LogitsProcessor lp(seed, 1.0, top_p > 0 ? std::optional<double>(top_p) : std::nullopt,
                                    top_k ? std::optional<size_t>(top_k) : std::nullopt);
        const std::vector<float> one(1, 1.0f);
        for (long i = 0; i < skip; i++) (void)lp.sample_prs(one.data(), 1);          // one word of the stream each
        for (long i = 0; i < draws; i++) {
            const uint32_t tok = lp.sample_prs(prs.data(), prs.size());
            std::printf("%u %zu\n", tok, lp.kept());
        }
        // the constructor refuses a NaN top_p, as the ABI does
        bool refused = false;
        try { fastllm::LogitsProcessor bad(0, 1.0, std::nan("")); } catch (const fastllm::Error &) { refused = true; }
        if (!refused) { std::fprintf(stderr, "NaN top_p was accepted\n"); return 1; }
    } catch (const std::exception &e) { std::fprintf(stderr, "error: %s\n", e.what()); return 1; }
    std::printf("host top-p driver done\n");
    return 0;
}
