// Prints gemv_resid_edge() for the cases on the command line: groups of ten integers
//   N K Nc R cus force_blocks force_waves bf16 one_shard compute_weights   ->   one line "yes blocks waves" each
// (blocks, waves: the producer's grid).  "sweep K Nc R cus" as the only arguments: one such line for every N = 8, 16 ... 8192.
// Compiled with the host compiler alone (tests/test_gemv_resid_plan.py): the header must not need HIP.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "gemv_geometry.h"

static void one(const fl::GemvResidEdge &e) {
    fl::GemvGeometry g{0, 0};
    const bool yes = fl::gemv_resid_edge(e, &g);
    printf("%d %d %d\n", yes ? 1 : 0, g.blocks, g.waves);
}

int main(int argc, char **argv) {
    if (argc == 6 && !strcmp(argv[1], "sweep")) {
        for (int64_t N = 8; N <= 8192; N += 8) {
            fl::GemvResidEdge e;
            e.N = N; e.K = atoll(argv[2]); e.Nc = atoll(argv[3]); e.R = atoi(argv[4]); e.cus = atoi(argv[5]);
            one(e);
        }
        return 0;
    }
    if ((argc - 1) % 10) return 2;
    for (int i = 1; i + 9 < argc; i += 10) {
        fl::GemvResidEdge e;
        e.N = atoll(argv[i]); e.K = atoll(argv[i + 1]); e.Nc = atoll(argv[i + 2]); e.R = atoi(argv[i + 3]); e.cus = atoi(argv[i + 4]);
        e.force_blocks = atoi(argv[i + 5]); e.force_waves = atoi(argv[i + 6]);
        e.bf16 = atoi(argv[i + 7]) != 0; e.one_shard = atoi(argv[i + 8]) != 0; e.compute_weights = atoi(argv[i + 9]) != 0;
        one(e);
    }
    return 0;
}
