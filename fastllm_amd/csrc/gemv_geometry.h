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

// the grid launch_gemv runs an N x K bf16 matrix on, R rows per row group: gemv_geometry with its floor of four waves
inline GemvGeometry gemv_stream_geometry(int64_t N, int64_t K, int R, int cus) {
    GemvGeometry g = gemv_geometry((N + R - 1) / R, ((size_t)K * 2 + 15) & ~(size_t)15, cus, 0, 0);
    if (g.waves < 4) g.waves = 4;
    return g;
}

// One producer -> RMSNorm -> consumer edge of a decode step: may the producer (o_proj / down_proj, [N, K]) finish the residual add,
// v * w_next and the chunk sums of squares in its epilogue (EPI_RESID), and the consumer ([Nc, N]: gate/up, the next QKV projection
// or lm_head) stage the ready vector (PRO_XS)?  Everything else keeps the consumer's PRO_NORM prologue.
struct GemvResidEdge {
    int64_t N = 0, K = 0;                     // the producer's matrix
    int64_t Nc = 0;                           // rows of the consumer's matrix (device layout: gate/up padded to whole 32s)
    int R = 2;                                // rows per row group of both launches (fl_tune "gemv_r")
    int cus = 256;
    bool bf16 = true, one_shard = true, compute_weights = true;   // a bf16 model on one GPU that streams the compute-dtype weights
    int force_blocks = 0, force_waves = 0;    // fl_tune "gemv_blocks" / "gemv_waves"
};
// *producer (if given): the grid the producer then runs on
inline bool gemv_resid_edge(const GemvResidEdge &e, GemvGeometry *producer = nullptr) {
    if (!e.bf16 || !e.one_shard || !e.compute_weights || e.force_blocks != 0 || e.force_waves != 0) return false;
    if (e.N <= 0 || e.K <= 0 || e.Nc <= 0 || e.R <= 0 || e.N % 8 || e.K % 8 || e.N % e.R) return false;
    const GemvGeometry p = gemv_stream_geometry(e.N, e.K, e.R, e.cus);
    if (producer) *producer = p;
    // the grid covers N exactly, one row group per wave; a workgroup's rows are whole 8-element chunks of the consumer's K
    if ((int64_t)p.blocks * p.waves * e.R != e.N || (p.waves * e.R) % 8 != 0) return false;
    // the consumer stages one chunk per thread
    const GemvGeometry c = gemv_stream_geometry(e.Nc, e.N, e.R, e.cus);
    return e.N / 8 <= (int64_t)c.waves * 64;
}

}  // namespace fl
