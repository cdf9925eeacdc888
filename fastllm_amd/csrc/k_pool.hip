// k_pool.hip -- pool_rows_kernel: the tail of a decoder-model embedding call (fl_batch_embed, fl_op_pool_rows).  Behind the final
// launch_rmsnorm_add the fp32 residual stream x [T][h] and every row's 1/rms are in memory; an embedding request wants a member's
// pooled final hidden state, not its logits, so this launch stands where lm_head and token selection stand in a prefill.
//
// For row t the hidden state is hid[t][j] = (x[t][j] * inv_rms[t]) * w[j], both products rounded to fp32 on their own (no FMA), so
// that a numpy float32 restatement reproduces the bits.  Per member: LAST / FIRST take one row; MEAN adds the member's rows in row
// order from +0, one rounded add per row, and divides once by (float)count; NONE makes every row a member of its own.
//
// Lanes own columns: a workgroup is ONE wave that owns a member and a chunk of 256 columns, four consecutive ones per lane -- one
// 16-byte load per lane and row, 1 KiB contiguous per wave -- and walks the member's rows sequentially, sixteen rows requested ahead
// of the first add.  The row order of MEAN leaves no parallelism over rows, so a long member is spread over its column chunks only:
// 16 workgroups at h = 4096.  That is the slow case, MEAN over one member of 8192 rows (128 MB): 16 waves of a 256-CU device with
// 16 KiB in flight each; profiles/r17/embed_decoder.txt has its time, a fraction of a millisecond behind a forward of 8192 tokens.
// Narrower chunks (128 columns as 8-byte loads, 64 as 4-byte loads) would put two or four times as many waves on it at half or a
// quarter of the bytes per request, and would make the common packs (tens of members, a few hundred rows each: hundreds of
// workgroups already) issue two or four times as many loads; the 16-byte form is kept.  Only the first `dims` columns are computed.  Where h is not a multiple of 4, a buffer is not 16-byte
// aligned or a lane's four columns straddle dims, that lane goes one column at a time (as k_logit_rules.hip does); the output rows
// [dims] are vector-stored only where their address allows.
//
// The L2 norm spans a member's chunks.  Each workgroup leaves its partial sum of squares (a fixed shuffle tree over the wave) in
// part[member][chunk], and a SECOND small launch adds the partials in chunk order and divides the vector.  The alternative -- an
// integer ticket per member and the last arriver scaling, as verify_packed_kernel does -- saves that launch (a few microseconds
// behind a whole forward) at the price of fences, a ticket array that NONE would need per row (8192 words to keep at zero) and the
// last workgroup of a member re-reading what others wrote; two launches need no ordering between workgroups at all, and the bits
// cannot depend on arrival order.  No atomics anywhere.
#include "kernels.h"

// Every product and sum below is an operation of its own: hipcc's default (-ffp-contract=fast) would contract the MEAN step
// acc + (x * inv_rms) * w into an FMA, whose bits a float32 restatement does not reproduce -- and the __fmul_rn / __fadd_rn of the
// HIP headers do not help: they are inline functions around the plain operators, carry the headers' contraction flag and fuse after
// inlining.  So the arithmetic below is written with the operators themselves, under this pragma; division and square root are the
// correctly rounded ones (hipcc's default).  The sum of squares asks for its FMA explicitly.
#pragma clang fp contract(off)

namespace fl {

constexpr int kPoolVec = 4, kPoolCols = 64 * kPoolVec, kPoolAhead = 16;

__global__ __launch_bounds__(64) void pool_rows_kernel(const float *__restrict__ x, const float *__restrict__ inv_rms, const float *__restrict__ w,
                                                       const int *__restrict__ seq_off, const int *__restrict__ seq_cnt, int h, int dims, int pooling,
                                                       float *__restrict__ part, float *__restrict__ out) {
    const int s = blockIdx.x, chunk = blockIdx.y, lane = threadIdx.x;
    size_t row0 = (size_t)s;
    int n = 1;
    if (pooling != FL_POOL_NONE) {
        const int off = seq_off[s], cnt = seq_cnt[s];
        row0 = (size_t)(pooling == FL_POOL_LAST ? off + cnt - 1 : off);
        if (pooling == FL_POOL_MEAN) n = cnt;
    }
    const int j0 = chunk * kPoolCols + lane * kPoolVec;
    const int nj = min(kPoolVec, dims - j0);                       // this lane's columns (<= 0: none)
    const bool vec = nj == kPoolVec && (h & 3) == 0 && ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(w)) & 15) == 0;
    float wv[kPoolVec] = {0.f, 0.f, 0.f, 0.f}, p[kPoolVec] = {0.f, 0.f, 0.f, 0.f};
    if (vec) {
        const float4v t = *reinterpret_cast<const float4v *>(w + j0);
#pragma unroll
        for (int c = 0; c < kPoolVec; c++) wv[c] = t[c];
    } else {
        for (int c = 0; c < nj; c++) wv[c] = w[j0 + c];
    }
    auto load_row = [&](size_t r, float (&v)[kPoolVec]) {
        const float *xr = x + r * (size_t)h + j0;
        if (vec) {
            const float4v t = *reinterpret_cast<const float4v *>(xr);
#pragma unroll
            for (int c = 0; c < kPoolVec; c++) v[c] = t[c];
        } else {
#pragma unroll
            for (int c = 0; c < kPoolVec; c++) v[c] = c < nj ? xr[c] : 0.f;
        }
    };
    if (pooling != FL_POOL_MEAN) {
        float v[kPoolVec];
        load_row(row0, v);
        const float ir = inv_rms[row0];
#pragma unroll
        for (int c = 0; c < kPoolVec; c++) p[c] = (v[c] * ir) * wv[c];
    } else {
        for (int r = 0; r < n; r += kPoolAhead) {                  // (n is uniform over the workgroup)
            float v[kPoolAhead][kPoolVec], ir[kPoolAhead];
#pragma unroll
            for (int u = 0; u < kPoolAhead; u++)
                if (r + u < n) { load_row(row0 + (size_t)(r + u), v[u]); ir[u] = inv_rms[row0 + (size_t)(r + u)]; }
#pragma unroll
            for (int u = 0; u < kPoolAhead; u++)
                if (r + u < n) {
#pragma unroll
                    for (int c = 0; c < kPoolVec; c++) p[c] = p[c] + (v[u][c] * ir[u]) * wv[c];
                }
        }
        const float cnt = (float)n;
#pragma unroll
        for (int c = 0; c < kPoolVec; c++) p[c] = p[c] / cnt;
    }
    float *o = out + (size_t)s * dims + j0;
    if (nj == kPoolVec && (reinterpret_cast<uintptr_t>(o) & 15) == 0) {
        float4v t;
#pragma unroll
        for (int c = 0; c < kPoolVec; c++) t[c] = p[c];
        *reinterpret_cast<float4v *>(o) = t;
    } else {
        for (int c = 0; c < nj; c++) o[c] = p[c];
    }
    if (!part) return;
    float ss = 0.f;
#pragma unroll
    for (int c = 0; c < kPoolVec; c++) if (c < nj) ss = fmaf(p[c], p[c], ss);
    ss = wave_sum(ss);
    if (lane == 0) part[(size_t)s * gridDim.y + chunk] = ss;
}

// out[s][:] /= sqrt(part[s][0] + part[s][1] + ...), the partials added in chunk order; a zero vector stays zero
__global__ __launch_bounds__(256) void pool_scale_kernel(const float *__restrict__ part, int n_chunk, int dims, float *__restrict__ out) {
    const int s = blockIdx.x;
    float ss = 0.f;
    for (int c = 0; c < n_chunk; c++) ss = ss + part[(size_t)s * n_chunk + c];
    if (ss == 0.f) return;
    const float norm = __fsqrt_rn(ss);
    float *o = out + (size_t)s * dims;
    for (int j = threadIdx.x; j < dims; j += 256) o[j] = o[j] / norm;
}

int pool_rows_chunks(int64_t dims) { return (int)((dims + kPoolCols - 1) / kPoolCols); }

int launch_pool_rows(Launcher &L, const float *x, const float *inv_rms, const float *w, const int *seq_off, const int *seq_cnt, int n_out,
                     int64_t h, int64_t dims, int pooling, bool normalize, float *part, float *out) {
    if (h < 1 || h > 65536 || dims < 1 || dims > h || n_out < 1 || n_out > (1 << 20)) FL_FAIL(FL_ERR_BAD_ARGUMENT, "pool_rows: bad shape");
    if (pooling < FL_POOL_LAST || pooling > FL_POOL_NONE) FL_FAIL(FL_ERR_BAD_ARGUMENT, "pool_rows: unknown pooling %d", pooling);
    if (!x || !inv_rms || !w || !out || (pooling != FL_POOL_NONE && (!seq_off || !seq_cnt)) || (normalize && !part))
        FL_FAIL(FL_ERR_BAD_ARGUMENT, "pool_rows: null argument");
    const int nch = pool_rows_chunks(dims);
    const char *tag = L.tag;
    L.tag = "pool";
    // algorithmic bytes: one row per output (MEAN: the caller's rows are not known here), the vector out
    int rc = L.launch(KC_CONVERT, (double)n_out * dims * 8, 0, pool_rows_kernel, dim3((unsigned)n_out, (unsigned)nch), dim3(64), 0, x, inv_rms, w, seq_off,
                      seq_cnt, (int)h, (int)dims, pooling, normalize ? part : nullptr, out);
    if (rc == FL_OK && normalize) {
        L.tag = "pool_scale";
        rc = L.launch(KC_CONVERT, (double)n_out * dims * 8, 0, pool_scale_kernel, dim3((unsigned)n_out), dim3(256), 0, (const float *)part, nch, (int)dims, out);
    }
    L.tag = tag;
    return rc;
}

}  // namespace fl
