// Prints the prefill attention plans (attn_prefill_plan.h) for the cases on the command line.  A case is
//   s T H Hkv d force scale_positive cus  pf32_min_t pf32_ks2 pf32_paired pf_waves pf_stages pf_ksplit
//       -> "32 nw ksf TB paired gsub grid_x grid_y block lds tag"   or   "16 TT ks nst grid_x grid_y block lds"
//   p H Hkv d  pf32_min_t pf32_ks2 pf32_paired pf_waves pf_stages pf_ksplit  n count_1 .. count_n
//       -> "TT ks"
// Compiled with the host compiler alone (tests/test_attn_prefill_plan.py): the header must not need HIP.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "attn_prefill_plan.h"

int main(int argc, char **argv) {
    int i = 1;
    auto next = [&]() { return i < argc ? atoll(argv[i++]) : 0; };
    auto tune = [&]() { fl::AttnPrefillTune t; t.pf32_min_t = (int)next(); t.pf32_ks2 = (int)next(); t.pf32_paired = (int)next();
                        t.pf_waves = (int)next(); t.pf_stages = (int)next(); t.pf_ksplit = (int)next(); return t; };
    while (i < argc) {
        const char *kind = argv[i++];
        if (!strcmp(kind, "s")) {
            if (argc - i < 13) return 2;
            const long long T = next(), H = next(), Hkv = next(), d = next();
            const int force = (int)next(), pos = (int)next(), cus = (int)next();
            const fl::AttnPrefillPlan p = fl::plan_attn_prefill(T, H, Hkv, d, force, pos != 0, cus, tune());
            if (p.rows == 32) printf("32 %d %d %d %d %d %u %u %d %zu %s\n", p.nw, p.ksf, p.TB, p.paired, p.gsub, p.grid_x, p.grid_y, p.block, p.lds, p.tag);
            else printf("16 %d %d %d %u %u %d %zu\n", p.TT, p.ks, p.nst, p.grid_x, p.grid_y, p.block, p.lds);
        } else if (!strcmp(kind, "p")) {
            if (argc - i < 10) return 2;
            const long long H = next(), Hkv = next(), d = next();
            const fl::AttnPrefillTune t = tune();
            const int n = (int)next();
            if (argc - i < n) return 2;
            std::vector<int> counts;
            for (int k = 0; k < n; k++) counts.push_back((int)next());
            const fl::AttnPackedPlan p = fl::plan_attn_prefill_packed(H, Hkv, d, counts.data(), n, t);
            printf("%d %d\n", p.TT, p.ks);
        } else {
            return 2;
        }
    }
    return 0;
}
