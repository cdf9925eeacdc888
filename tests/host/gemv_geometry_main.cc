// Prints gemv_geometry() for the cases on the command line: groups of five integers
//   ngroups lds_bytes cus force_blocks force_waves   ->   one line "blocks waves" each.
// Compiled with the host compiler alone (tests/test_gemv_geometry.py): the header must not need HIP.
#include <stdio.h>
#include <stdlib.h>

#include "gemv_geometry.h"

int main(int argc, char **argv) {
    if ((argc - 1) % 5) return 2;
    for (int i = 1; i + 4 < argc; i += 5) {
        const fl::GemvGeometry g = fl::gemv_geometry(atoll(argv[i]), (size_t)atoll(argv[i + 1]), atoi(argv[i + 2]), atoi(argv[i + 3]), atoi(argv[i + 4]));
        printf("%d %d\n", g.blocks, g.waves);
    }
    return 0;
}
