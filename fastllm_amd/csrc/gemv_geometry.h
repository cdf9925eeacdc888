// gemv_geometry.h -- the grid of a decode weight stream (k_gemv.hip, k_gemv_w8.hip): plain C++, no HIP, so that
// tests/test_gemv_geometry.py compiles it with the host compiler alone.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace fl {

struct GemvGeometry { int blocks, waves; };

// (workgroups, waves per workgroup) for `ngroups` row groups on `cus` CUs: one workgroup per CU (or two), 4..12 waves each,
// chosen so that every wave gets the same number of row groups (a ragged last round costs 1/rounds of the kernel), everything
// resident at once (<= 12 waves per CU at 170 VGPRs, the workgroups' LDS side by side), and as many waves per CU as that
// allows.  A forced (blocks, waves) pair, both > 0, is returned as given (fl_tune "gemv_blocks" / "gemv_waves"; the FP8 stream
// passes 0, 0).
inline GemvGeometry gemv_geometry(int64_t ngroups, size_t lds_bytes, int cus, int force_blocks, int force_waves) {
    if (force_blocks > 0 && force_waves > 0) return {force_blocks, force_waves};
    if (ngroups <= (int64_t)cus * 4) return {(int)((ngroups + 3) / 4), 4};   // small matrix: 4-wave workgroups, one group per wave
    double best = -1.0;
    GemvGeometry g{cus, 8};
    for (int mult = 1; mult <= 2; mult++) {
        for (int w = 12; w >= 4; w--) {
            if (mult * w > 12 || (size_t)mult * lds_bytes > 150 * 1024) continue;
            const int64_t wt = (int64_t)cus * mult * w;
            const int64_t per = (ngroups + wt - 1) / wt;
            const double eff = (double)ngroups / (double)(per * wt);
            // prefer balance, then more waves per CU (latency hiding), then fewer workgroups
            const double score = eff + 1e-3 * (mult * w) / 12.0 - 1e-4 * mult;
            if (score > best) { best = score; g = {cus * mult, w}; }
        }
    }
    return g;
}

}  // namespace fl
