// k_gemm_rows_w8.hip -- the 2-16-row weight stream over FP8 weights: Y[T,N] = rs[t] * s[n] * (X[T,K] . q[N,K]^T) (+ bias[n]).
//
// The multi-row sibling of gemv_w8_kernel (k_gemv_w8.hip; same format: q OCP e4m3fn [N,K] row-major, s[n] a power of two), for the
// verify step of speculative decoding: a forward of 2-16 rows over 7 B weights is a weight stream, and on an FL_WEIGHTS_E4M3_ROW model
// the e4m3 bytes are half the stream of the bf16 image s * q that launch_linear reads.  What it does:
//   - weights never touch LDS.  A wave owns 16 weight rows at a time (a gate | up pair: 32); lane (r = lane & 15, g = lane >> 4)
//     loads 16 bytes = 16 weights of row n0 + r at k0 + 16 g, non-temporal, straight to VGPRs: one wave instruction is 16 rows x
//     64 B, and the wave's consecutive instructions walk K, so a 128-byte line is consumed by one wave back to back.  The wave's
//     (row group, K block) items form one stream, a block (U instructions per 16 rows) ahead in a second register buffer; every
//     load is unconditional (counted vmcnt waits): past the end of K a lane re-reads the last chunk, a row past N re-reads row N - 1.
//   - conversion is the GEMV's: v_cvt_scalef32_pk_bf16_fp8 with scale 1.0, exact.  The 16 bytes become two 8-element bf16 MFMA
//     operands (bytes 0-7 | bytes 8-15), so a loaded 16 bytes feed two v_mfma_f32_16x16x32_bf16: tokens are the A rows, the 16 weight
//     rows the B columns.  The x fragment of lane (t = lane & 15, g) is x[t][k0 + 16 g + 0..7] for the first and + 8..15 for the
//     second: both operands see the same permutation of K inside a 64-wide block, which a dot product does not notice.  One fp32
//     16 x 16 accumulator per wave (two for gate | up) covers all token rows: C/D col = lane & 15 (weight row), row = 4 g + reg (token).
//   - x is staged once per workgroup as [T][Ks + 8] bf16, the T real rows only (lanes with t >= T read row 0 and select zero).  The
//     row stride is an odd number of 16-byte units, so the 16 lanes of a g -- 16 rows, one column -- hit 16 different 16-byte bank
//     groups and a wave's ds_read_b128 is conflict-free.  The first weight block is requested before x is staged.
//   - K slices: T * (Ks + 8) * 2 bytes must fit the 160 KB of a CU (the kernel has no static LDS).  A longer K -- or a matrix with too
//     few row groups to occupy the chip -- is cut over blockIdx.y into nks slices, each a multiple of 64, that write fp32 slabs
//     [nks][T][N] as gemv_batch_kernel does; the rmsnorm_add / rope_kv launch behind it sums them in slab order.  Only the plain
//     epilogue without bias may be sliced, and only when the caller takes slabs (gemm_rows_w8_plan decides; 0 = not served).
//   - epilogues: EPI_F32 acc * s[n] * rs[t] + bias[n]; EPI_GATEUP silu(g) * u as bf16 with the index map of skinny_epilogue.  s is a
//     power of two, so acc * s is exact and the rows equal the bf16-image rows up to fp32 summation order.  The scales (and bias) of
//     a row group are requested when the group starts.
// K must be a multiple of 16 (a lane's load).
#include <stdlib.h>

#include <algorithm>

#include "gemv_geometry.h"
#include "kernels.h"

namespace fl {

constexpr int kRowsW8MaxThreads = 768;              // 12 waves: 170 VGPRs per lane
constexpr size_t kRowsW8Lds = 160 * 1024;           // x rows of a workgroup: all of a CU's LDS (no static arrays)
constexpr int kRowsW8Pad = 8;                       // bf16 elements: (Ks + 8) / 8 is odd (Ks % 16 == 0)
typedef __bf16 bf16x8w __attribute__((ext_vector_type(8)));

struct RowsW8Args {
    const uint8_t *q; const float *s;               // [N,K] e4m3, [N]
    const bf16_t *x;                                // [T,K]
    const float *rs, *bias;                         // [T] / [N], or null
    void *out;                                      // EPI_F32: float [nks][T][N]; EPI_GATEUP: bf16 [T][N/2]
    int T, N, K, Ks;                                // Ks: columns per slice (K, or a multiple of 64)
};

// eight e4m3 (two dwords) as one bf16 MFMA operand, element i = byte i
__device__ inline bf16x8w e4m3x8_to_bf16x8(unsigned lo, unsigned hi) {
    uint4v r;
    r[0] = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(lo, 1.0f, false));
    r[1] = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(lo, 1.0f, true));
    r[2] = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(hi, 1.0f, false));
    r[3] = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(hi, 1.0f, true));
    return __builtin_bit_cast(bf16x8w, r);
}

template <int U, int EPI>
__global__ __launch_bounds__(kRowsW8MaxThreads) void gemm_rows_w8_kernel(const RowsW8Args a) {
    constexpr int NT = EPI == EPI_GATEUP ? 2 : 1;    // 16-row tiles of a row group
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    bf16_t *xs = reinterpret_cast<bf16_t *>(lds_raw);
    const int T = a.T, N = a.N, K = a.K;
    const int tid = threadIdx.x, lane = tid & 63, nthr = blockDim.x, nwv = nthr >> 6;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r16 = lane & 15, g = lane >> 4;
    const int k0 = blockIdx.y * a.Ks, Ksl = min(a.Ks, K - k0);                       // this workgroup's slice of K: a multiple of 16
    const int stride = a.Ks + kRowsW8Pad;
    const int nchunk = Ksl >> 4;                                                    // 16-weight chunks of a row's slice
    const int nb = ((Ksl + 63) / 64 + U - 1) / U;                                   // K blocks per row group (the last may be partial)
    const int ngroups = (N + 16 * NT - 1) / (16 * NT);
    const int gw = blockIdx.x * nwv + wave, nw = gridDim.x * nwv;
    const int n_items = gw < ngroups ? (ngroups - gw + nw - 1) / nw * nb : 0;      // this wave's items

    typedef uint4v Buf[NT][U];
    int lg = gw, lb = 0;                                                            // load stream: next item = (row group, block)
    auto load_next = [&](Buf &buf) {
        const int grp = min(lg, ngroups - 1);
#pragma unroll
        for (int j = 0; j < NT; j++) {
            const uint8_t *wr = a.q + (size_t)min(grp * 16 * NT + 16 * j + r16, N - 1) * K + k0;
#pragma unroll
            for (int u = 0; u < U; u++)
                buf[j][u] = __builtin_nontemporal_load(reinterpret_cast<const uint4v *>(wr + (size_t)min(4 * (U * lb + u) + g, nchunk - 1) * 16));
        }
        if (++lb == nb) { lb = 0; lg += nw; }
    };

    Buf pre;
    load_next(pre);
    {   // the T real rows of x, this slice's columns
        const int nch8 = Ksl >> 3, total = T * nch8;
#pragma unroll 4
        for (int i = tid; i < total; i += nthr) {
            const int t = i / nch8, c = i - t * nch8;
            *reinterpret_cast<uint4v *>(xs + t * stride + c * 8) = *reinterpret_cast<const uint4v *>(a.x + (size_t)t * K + k0 + c * 8);
        }
        __syncthreads();
    }
    const bool tok = r16 < T;
    const bf16_t *xrow = xs + (tok ? r16 : 0) * stride;

    // operands of the epilogue: the tokens' row scales once, the weight rows' scales and bias when a row group starts
    float rsv[4];
#pragma unroll
    for (int rg = 0; rg < 4; rg++) rsv[rg] = (a.rs && 4 * g + rg < T) ? a.rs[4 * g + rg] : 1.0f;
    float wsc[NT], bv = 0.f;
    auto group_prefetch = [&](int grp) {
#pragma unroll
        for (int j = 0; j < NT; j++) {
            const int n = grp * 16 * NT + 16 * j + r16;
            wsc[j] = n < N ? a.s[n] : 0.f;
            if constexpr (EPI == EPI_F32) bv = (a.bias && n < N) ? a.bias[n] : 0.f;
        }
    };
    if (gw < ngroups) group_prefetch(gw);

    float4v acc[NT];
#pragma unroll
    for (int j = 0; j < NT; j++) acc[j] = float4v{0.f, 0.f, 0.f, 0.f};

    auto finish_group = [&](int grp) {
        const int n = grp * 16 * NT + r16;                                          // EPI_GATEUP: the gate row; up = n + 16
#pragma unroll
        for (int rg = 0; rg < 4; rg++) {
            const int m = 4 * g + rg;
            if constexpr (EPI == EPI_GATEUP) {
                if (m < T && n + 16 < N) {
                    const int qq = (n >> 5) * 16 + (n & 15);
                    const float gt = acc[0][rg] * wsc[0] * rsv[rg], up = acc[NT - 1][rg] * wsc[NT - 1] * rsv[rg];
                    reinterpret_cast<bf16_t *>(a.out)[(size_t)m * (N / 2) + qq] = float_to_bf16_bits(gt / (1.0f + expf(-gt)) * up);
                }
            } else {
                if (m < T && n < N) reinterpret_cast<float *>(a.out)[((size_t)blockIdx.y * T + m) * N + n] = acc[0][rg] * wsc[0] * rsv[rg] + bv;
            }
        }
#pragma unroll
        for (int j = 0; j < NT; j++) acc[j] = float4v{0.f, 0.f, 0.f, 0.f};
    };

    int cg = gw, cb = 0;                                                            // consume stream
    auto consume = [&](const Buf &buf) {
        if (cb == 0 && cg != gw) group_prefetch(cg);
#pragma unroll
        for (int u = 0; u < U; u++) {
            const int kl = 64 * (U * cb + u) + 16 * g;                              // this lane's 16 columns, inside the slice
            const bf16_t *xp = xrow + min(kl, Ksl - 16);
            const unsigned keep = (tok && kl < Ksl) ? ~0u : 0u;                      // no such token / past the end of K: zero (a mask, not a branch)
            const uint4v xa = *reinterpret_cast<const uint4v *>(xp) & keep, xb = *reinterpret_cast<const uint4v *>(xp + 8) & keep;
#pragma unroll
            for (int j = 0; j < NT; j++) {
                const uint4v w = buf[j][u];
                acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8w, xa), e4m3x8_to_bf16x8(w[0], w[1]), acc[j], 0, 0, 0);
                acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8w, xb), e4m3x8_to_bf16x8(w[2], w[3]), acc[j], 0, 0, 0);
            }
        }
        if (++cb == nb) { finish_group(cg); cb = 0; cg += nw; }
    };
    Buf nxt;
    int t = 0;
#pragma nounroll
    for (; t + 2 < n_items; t += 2) {
        load_next(nxt);
        consume(pre);
        load_next(pre);
        consume(nxt);
    }
    if (n_items - t == 2) { load_next(nxt); consume(pre); consume(nxt); }
    else if (n_items - t == 1) consume(pre);
}

static size_t rows_w8_lds(int64_t T, int64_t Ks) { return (size_t)T * (size_t)(Ks + kRowsW8Pad) * 2; }
// the slice length that cuts K into about `nks` slices: K itself, or a multiple of 64
static int64_t rows_w8_slice(int64_t K, int nks) { return nks <= 1 ? K : ((K + nks - 1) / nks + 63) / 64 * 64; }

// the slices of a product (0: not served) and the columns of one
static int rows_w8_slices(int64_t T, int64_t N, int64_t K, int epi, bool bias, int max_split, int64_t *Ks_out) {
    if (T < 2 || T > 16 || N <= 0 || N > (1 << 24) || K < 16 || K % 16 || K > (1 << 24)) return 0;
    if (epi != EPI_F32 && epi != EPI_GATEUP) return 0;
    if (epi == EPI_GATEUP && (N % 32 || bias)) return 0;
    const int cap = (epi == EPI_F32 && !bias && max_split > 1) ? max_split : 1;      // slabs: the plain epilogue, when the caller sums them
    int nks = 1;
    while (nks <= cap && rows_w8_lds(T, rows_w8_slice(K, nks)) > kRowsW8Lds) nks++;  // the x rows of a slice must fit LDS
    if (nks > cap) return 0;
    // few row groups (QKV, o_proj, down_proj: one or two per CU): more slices put more waves on the stream, as long as a slice
    // keeps at least eight 64-column blocks
    const int64_t ngroups = (N + 15) / 16, waves = (int64_t)device_cu_count() * 8;
    while (nks < cap && ngroups * nks < waves && (K / 64) / (nks + 1) >= 8) nks++;
    const int64_t Ks = rows_w8_slice(K, nks);
    if (Ks_out) *Ks_out = Ks;
    return (int)((K + Ks - 1) / Ks);
}
int gemm_rows_w8_plan(int64_t T, int64_t N, int64_t K, int epi, bool bias, int max_split) { return rows_w8_slices(T, N, K, epi, bias, max_split, nullptr); }

template <int U, int EPI>
static int launch_rows_w8_ue(Launcher &L, const RowsW8Args &a, int nks) {
    constexpr int NT = EPI == EPI_GATEUP ? 2 : 1;
    auto kern = gemm_rows_w8_kernel<U, EPI>;
    const size_t lds = rows_w8_lds(a.T, a.Ks);
    FL_TRY(raise_dynamic_lds(reinterpret_cast<const void *>(kern), lds));
    // row groups over waves by the rule of the decode streams (gemv_geometry.h), per slice
    const GemvGeometry geo = gemv_geometry(((int64_t)a.N + 16 * NT - 1) / (16 * NT), lds, device_cu_count(), 0, 0);
    char tag[32];
    snprintf(tag, sizeof tag, "rows%d,%dx%d%s,w8", a.T, a.N, a.K, EPI == EPI_GATEUP ? ",glu" : (nks > 1 ? ",splitK" : ""));
    Launcher LL = L; LL.tag = tag;
    return LL.launch(KC_GEMM_MFMA, (double)a.N * a.K + 4.0 * a.N + 2.0 * a.T * a.K, 2.0 * a.T * a.N * a.K, kern, dim3((unsigned)geo.blocks, (unsigned)nks),
                     dim3((unsigned)geo.waves * 64), lds, a);
}

int launch_gemm_rows_w8(Launcher &L, const uint8_t *q, const float *s, const void *x, const float *bias, void *y, int64_t T, int64_t N,
                        int64_t K, int epi, const float *row_scale, int max_split, int *n_split_out) {
    if (n_split_out) *n_split_out = 1;
    if (!q || !s || !x || !y) FL_FAIL(FL_ERR_BAD_ARGUMENT, "launch_gemm_rows_w8: null argument");
    int64_t Ks = 0;
    const int nks = rows_w8_slices(T, N, K, epi, bias != nullptr, n_split_out ? max_split : 1, &Ks);
    if (!nks) FL_FAIL(FL_ERR_UNSUPPORTED, "launch_gemm_rows_w8: %lld x %lld x %lld (epilogue %d) is not served: 2..16 rows, K a multiple of 16, x rows within LDS", (long long)T, (long long)N, (long long)K, epi);
    FL_TRY(rs_parts_to_vector(L, row_scale, T));       // (a residual epilogue may have left 1/rms as partial sums)
    if (n_split_out) *n_split_out = nks;
    RowsW8Args a;
    a.q = q; a.s = s; a.x = reinterpret_cast<const bf16_t *>(x); a.rs = row_scale; a.bias = bias; a.out = y;
    a.T = (int)T; a.N = (int)N; a.K = (int)K; a.Ks = (int)Ks;
    // instructions per block U: the deepest whose padding of a row's 64-column instruction count stays within an eighth; a gate | up
    // pair holds two tiles per block, so half as deep (the same 64 VGPRs per buffer)
    const int ni = (int)((std::min<int64_t>(a.Ks, K) + 63) / 64);
    auto fits = [&](int u) { return ((ni + u - 1) / u * u - ni) * 8 <= ni; };
    if (epi == EPI_GATEUP) return fits(4) ? launch_rows_w8_ue<4, EPI_GATEUP>(L, a, nks) : launch_rows_w8_ue<2, EPI_GATEUP>(L, a, nks);
    if (fits(8)) return launch_rows_w8_ue<8, EPI_F32>(L, a, nks);
    return fits(4) ? launch_rows_w8_ue<4, EPI_F32>(L, a, nks) : launch_rows_w8_ue<2, EPI_F32>(L, a, nks);
}

}  // namespace fl
