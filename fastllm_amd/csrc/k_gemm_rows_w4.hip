// k_gemm_rows_w4.hip -- the 2-16-row weight stream over MXFP4 weights: Y[T,N] = rs[t] * (X[T,K] . W'[N,K]^T) (+ bias[n]),
// W'[n,k] = 2^(e[n, k / 32] - 127) * q[n,k].
//
// The multi-row sibling of gemv_w4_kernel (k_gemv_w4.hip; same format: q OCP e2m1 [N, K/2] row-major, low nibble first, one e8m0
// byte per block of 32 k) and the 4-bit sibling of gemm_rows_w8_kernel (k_gemm_rows_w8.hip), for the verify step of speculative
// decoding and for decode batches of up to 16 members on an FL_WEIGHTS_MXFP4 model: 2-16 rows over 7 B weights are a weight stream,
// and the nibbles are 4.25 / 16 of the bf16 image 2^e * q that launch_linear reads.  From the FP8 kernel it keeps the (row group,
// K block) item stream with a second register buffer one item ahead, the unconditional clamped loads under counted vmcnt waits, x
// staged once per workgroup as [T][Ks + 8] bf16 (lanes t >= T masked to zero), gemv_geometry for the grid, fp32 slabs [nks][T][N]
// for K slices, and the two epilogues (a gate | up pair: 32 consecutive device rows, two accumulators).  Its own:
//   - load map.  Lane (r = lane & 15, g = lane >> 4) loads 16 bytes = 32 weights = exactly one MX block, non-temporal, straight to
//     VGPRs: block 4 i + g of row n0 + r for the wave's instruction i.  An instruction is 16 rows x 64 contiguous bytes = 128 columns
//     of each row: the access pattern of the FP8 kernel at twice the weights per byte.
//   - conversion.  Dword j of the load (8 nibbles) goes through four v_cvt_scalef32_pk_bf16_fp4 (byte selects 0..3) and is one
//     8-element bf16 MFMA operand; the scale operand is the lane's own block scale, byte << 23 as a float (exact over the whole
//     exponent range, as in the GEMV).  A loaded 16 bytes feed FOUR v_mfma_f32_16x16x32_bf16, one per dword: tokens are the A rows,
//     the 16 weight rows the B columns.  The x fragment of MFMA j for lane (t, g) is x[t][128 i + 32 g + 8 j .. + 7] -- a lane reads
//     64 contiguous bytes of its x row per instruction -- so both operands see the same permutation of K inside a 128-column
//     instruction, which a dot product does not notice.  One fp32 16 x 16 accumulator covers all token rows (two for gate | up):
//     C/D col = lane & 15 (weight row), row = 4 g + reg (token).
//   - scales: a second stream in the kernel's own order.  A row's scales are stored in groups of 16 blocks (512 columns), each group
//     transposed 4 x 4: byte 16 J + 4 g + u of the row holds the scale of block 16 J + 4 u + g, so ONE dword load per lane gives the
//     scales of four consecutive instructions, requested with the data of the same item.  Row stride = ceil(K / 512) * 16 bytes
//     (rows_w4_scale_stride), slots past K / 32 hold 127 (2^0): a function of K alone, not of T, the slicing or the item depth.  (The
//     GEMV's stream order interleaves blocks c and c + 64 for some K and cannot be read this way; launch_mx4_group_scales makes this
//     order from that one.)
//   - an item is G groups of a row group's 16-row tiles: G = 1 (four instructions: 16 VGPRs of data per tile per buffer) or, the
//     plain epilogue only, G = 2.  K slices are multiples of 512 columns, so a slice starts on a group.  Past the end of K a lane
//     re-reads the row's last block with its x masked to zero; a row past N re-reads row N - 1.
//   - there is no per-row weight scale in the epilogue: EPI_F32 acc * rs[t] + bias[n]; EPI_GATEUP silu(g) * u as bf16 with the index
//     map of skinny_epilogue.  The rows equal the bf16-image rows up to fp32 summation order.
// K must be a multiple of 32 (a lane's load, one block).
#include <stdlib.h>

#include <algorithm>

#include "gemv_geometry.h"
#include "kernels.h"

namespace fl {

constexpr int kRowsW4MaxThreads = 768;              // 12 waves: 170 VGPRs per lane
constexpr size_t kRowsW4Lds = 160 * 1024;           // x rows of a workgroup: all of a CU's LDS (no static arrays)
constexpr int kRowsW4Pad = 8;                       // bf16 elements: (Ks + 8) / 8 is odd (Ks % 32 == 0)
// (kRowsW4Group, the 512 columns of a scale group, and e2m1x8_to_bf16x8: kernels.h, shared with k_gemm_rows64_w4.hip)

struct RowsW4Args {
    const uint8_t *q, *e;                           // [N, K/2] nibbles; the group-order scale stream, `es` bytes per row
    const bf16_t *x;                                // [T,K]
    const float *rs, *bias;                         // [T] / [N], or null
    void *out;                                      // EPI_F32: float [nks][T][N]; EPI_GATEUP: bf16 [T][N/2]
    int T, N, K, Ks, es;                            // Ks: columns per slice (K, or a multiple of 512)
};

template <int G, int EPI>
__global__ __launch_bounds__(kRowsW4MaxThreads) void gemm_rows_w4_kernel(const RowsW4Args a) {
    constexpr int NT = EPI == EPI_GATEUP ? 2 : 1;    // 16-row tiles of a row group
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    bf16_t *xs = reinterpret_cast<bf16_t *>(lds_raw);
    const int T = a.T, N = a.N, K = a.K;
    const int tid = threadIdx.x, lane = tid & 63, nthr = blockDim.x, nwv = nthr >> 6;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r16 = lane & 15, g = lane >> 4;
    const int k0 = blockIdx.y * a.Ks, Ksl = min(a.Ks, K - k0);                       // this workgroup's slice of K: a multiple of 32, k0 of 512
    const int stride = a.Ks + kRowsW4Pad;
    const int nblk = Ksl >> 5;                                                      // MX blocks of a row's slice
    const int ngs = (Ksl + kRowsW4Group - 1) / kRowsW4Group;                        // scale groups of a row's slice (the last may be partial)
    const int nb = (ngs + G - 1) / G;                                               // items per row group
    const int ngroups = (N + 16 * NT - 1) / (16 * NT);
    const int gw = blockIdx.x * nwv + wave, nw = gridDim.x * nwv;
    const int n_items = gw < ngroups ? (ngroups - gw + nw - 1) / nw * nb : 0;      // this wave's items

    struct Buf { uint4v w[NT][G][4]; unsigned e[NT][G]; };
    int lg = gw, lb = 0;                                                            // load stream: next item = (row group, block)
    auto load_next = [&](Buf &buf) {
        const int grp = min(lg, ngroups - 1);
#pragma unroll
        for (int j = 0; j < NT; j++) {
            const size_t row = (size_t)min(grp * 16 * NT + 16 * j + r16, N - 1);
            const uint8_t *wr = a.q + row * (size_t)(K >> 1) + (k0 >> 1);
            const uint8_t *er = a.e + row * (size_t)a.es + (k0 / kRowsW4Group) * 16 + 4 * g;
#pragma unroll
            for (int gi = 0; gi < G; gi++) {
                const int J = G * lb + gi;                                          // the group, inside the slice
#pragma unroll
                for (int u = 0; u < 4; u++)
                    buf.w[j][gi][u] = __builtin_nontemporal_load(reinterpret_cast<const uint4v *>(wr + (size_t)min(16 * J + 4 * u + g, nblk - 1) * 16));
                buf.e[j][gi] = __builtin_nontemporal_load(reinterpret_cast<const unsigned *>(er + (size_t)min(J, ngs - 1) * 16));
            }
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

    // operands of the epilogue: the tokens' row scales once, the weight rows' bias when a row group starts
    float rsv[4];
#pragma unroll
    for (int rg = 0; rg < 4; rg++) rsv[rg] = (a.rs && 4 * g + rg < T) ? a.rs[4 * g + rg] : 1.0f;
    float bv = 0.f;
    auto group_prefetch = [&](int grp) {
        if constexpr (EPI == EPI_F32) {
            const int n = grp * 16 + r16;
            bv = (a.bias && n < N) ? a.bias[n] : 0.f;
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
                    const float gt = acc[0][rg] * rsv[rg], up = acc[NT - 1][rg] * rsv[rg];
                    reinterpret_cast<bf16_t *>(a.out)[(size_t)m * (N / 2) + qq] = float_to_bf16_bits(gt / (1.0f + expf(-gt)) * up);
                }
            } else {
                if (m < T && n < N) reinterpret_cast<float *>(a.out)[((size_t)blockIdx.y * T + m) * N + n] = acc[0][rg] * rsv[rg] + bv;
            }
        }
#pragma unroll
        for (int j = 0; j < NT; j++) acc[j] = float4v{0.f, 0.f, 0.f, 0.f};
    };

    int cg = gw, cb = 0;                                                            // consume stream
    auto consume = [&](const Buf &buf) {
        if (cb == 0 && cg != gw) group_prefetch(cg);
#pragma unroll
        for (int gi = 0; gi < G; gi++) {
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const int blk = 16 * (G * cb + gi) + 4 * u + g;                      // this lane's block, inside the slice
                const bf16_t *xp = xrow + min(blk, nblk - 1) * 32;
                const unsigned keep = (tok && blk < nblk) ? ~0u : 0u;                // no such token / past the end of K: zero (a mask, not a branch)
                uint4v xf[4];
#pragma unroll
                for (int d = 0; d < 4; d++) xf[d] = *reinterpret_cast<const uint4v *>(xp + 8 * d) & keep;
#pragma unroll
                for (int j = 0; j < NT; j++) {
                    const float sc = __uint_as_float(((buf.e[j][gi] >> (8 * u)) & 0xffu) << 23);
                    const uint4v w = buf.w[j][gi][u];
#pragma unroll
                    for (int d = 0; d < 4; d++)
                        acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8q, xf[d]), e2m1x8_to_bf16x8(w[d], sc), acc[j], 0, 0, 0);
                }
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

int64_t rows_w4_scale_stride(int64_t K) { return (K + kRowsW4Group - 1) / kRowsW4Group * 16; }

static size_t rows_w4_lds(int64_t T, int64_t Ks) { return (size_t)T * (size_t)(Ks + kRowsW4Pad) * 2; }
// the slice length that cuts K into about `nks` slices: K itself, or a multiple of 512 (whole scale groups)
static int64_t rows_w4_slice(int64_t K, int nks) { return nks <= 1 ? K : ((K + nks - 1) / nks + kRowsW4Group - 1) / kRowsW4Group * kRowsW4Group; }

// the slices of a product (0: not served) and the columns of one: the rule of rows_w8_slices
static int rows_w4_slices(int64_t T, int64_t N, int64_t K, int epi, bool bias, int max_split, int64_t *Ks_out) {
    if (T < 2 || T > 16 || N <= 0 || N > (1 << 24) || K < 32 || K % 32 || K > (1 << 24)) return 0;
    if (epi != EPI_F32 && epi != EPI_GATEUP) return 0;
    if (epi == EPI_GATEUP && (N % 32 || bias)) return 0;
    const int cap = (epi == EPI_F32 && !bias && max_split > 1) ? max_split : 1;      // slabs: the plain epilogue, when the caller sums them
    int nks = 1;
    while (nks <= cap && rows_w4_lds(T, rows_w4_slice(K, nks)) > kRowsW4Lds) nks++;  // the x rows of a slice must fit LDS
    if (nks > cap) return 0;
    // few row groups (QKV, o_proj, down_proj: one or two per CU): more slices put more waves on the stream, as long as a slice
    // keeps at least two groups -- 1024 columns, the bytes per wave and row group that the FP8 rule's eight 64-column blocks are
    const int64_t ngroups = (N + 15) / 16, waves = (int64_t)device_cu_count() * 8;
    while (nks < cap && ngroups * nks < waves && (K / kRowsW4Group) / (nks + 1) >= 2) nks++;
    const int64_t Ks = rows_w4_slice(K, nks);
    if (Ks_out) *Ks_out = Ks;
    return (int)((K + Ks - 1) / Ks);
}
int gemm_rows_w4_plan(int64_t T, int64_t N, int64_t K, int epi, bool bias, int max_split) { return rows_w4_slices(T, N, K, epi, bias, max_split, nullptr); }

template <int G, int EPI>
static int launch_rows_w4_ge(Launcher &L, const RowsW4Args &a, int nks) {
    constexpr int NT = EPI == EPI_GATEUP ? 2 : 1;
    auto kern = gemm_rows_w4_kernel<G, EPI>;
    const size_t lds = rows_w4_lds(a.T, a.Ks);
    FL_TRY(raise_dynamic_lds(reinterpret_cast<const void *>(kern), lds));
    // row groups over waves by the rule of the decode streams (gemv_geometry.h), per slice
    const GemvGeometry geo = gemv_geometry(((int64_t)a.N + 16 * NT - 1) / (16 * NT), lds, device_cu_count(), 0, 0);
    char tag[32];
    snprintf(tag, sizeof tag, "rows%d,%dx%d%s,w4", a.T, a.N, a.K, EPI == EPI_GATEUP ? ",glu" : (nks > 1 ? ",splitK" : ""));
    Launcher LL = L; LL.tag = tag;
    return LL.launch(KC_GEMM_MFMA, (double)a.N * (a.K / 2 + a.es) + 2.0 * a.T * a.K, 2.0 * a.T * a.N * a.K, kern, dim3((unsigned)geo.blocks, (unsigned)nks),
                     dim3((unsigned)geo.waves * 64), lds, a);
}

int launch_gemm_rows_w4(Launcher &L, const uint8_t *q, const uint8_t *e, const void *x, const float *bias, void *y, int64_t T, int64_t N,
                        int64_t K, int epi, const float *row_scale, int max_split, int *n_split_out) {
    if (n_split_out) *n_split_out = 1;
    if (!q || !e || !x || !y) FL_FAIL(FL_ERR_BAD_ARGUMENT, "launch_gemm_rows_w4: null argument");
    int64_t Ks = 0;
    const int nks = rows_w4_slices(T, N, K, epi, bias != nullptr, n_split_out ? max_split : 1, &Ks);
    if (!nks) FL_FAIL(FL_ERR_UNSUPPORTED, "launch_gemm_rows_w4: %lld x %lld x %lld (epilogue %d) is not served: 2..16 rows, K a multiple of 32, x rows within LDS", (long long)T, (long long)N, (long long)K, epi);
    FL_TRY(rs_parts_to_vector(L, row_scale, T));       // (a residual epilogue may have left 1/rms as partial sums)
    if (n_split_out) *n_split_out = nks;
    RowsW4Args a;
    a.q = q; a.e = e; a.x = reinterpret_cast<const bf16_t *>(x); a.rs = row_scale; a.bias = bias; a.out = y;
    a.T = (int)T; a.N = (int)N; a.K = (int)K; a.Ks = (int)Ks; a.es = (int)rows_w4_scale_stride(K);
    if (epi == EPI_GATEUP) return launch_rows_w4_ge<1, EPI_GATEUP>(L, a, nks);
    // two groups per item where that pads a slice's group count by no more than an eighth (the rule of the FP8 kernel's depth)
    const int ng = (int)((std::min<int64_t>(a.Ks, K) + kRowsW4Group - 1) / kRowsW4Group);
    return (ng % 2) * 8 <= ng ? launch_rows_w4_ge<2, EPI_F32>(L, a, nks) : launch_rows_w4_ge<1, EPI_F32>(L, a, nks);
}

// ---- the group-order scale stream from the GEMV's stream (what the quantiser and launch_mx4_layout write) ---------------------
// one thread per (row, destination dword): the four scales of lane group g in group J, slots past K / 32 set to 127
__global__ __launch_bounds__(256) void mx4_group_scales_kernel(const uint8_t *__restrict__ es, int64_t N, int64_t K, int U, int64_t sstride, uint8_t *__restrict__ eo) {
    const int64_t per = (K + kRowsW4Group - 1) / kRowsW4Group * 4, i = (int64_t)blockIdx.x * 256 + threadIdx.x;   // dwords of a row
    if (i >= N * per) return;
    const int64_t row = i / per, d = i - row * per, J = d >> 2, nchunk = K >> 5;
    const int g = (int)(d & 3);
    unsigned word = 0;
#pragma unroll
    for (int u = 0; u < 4; u++) {
        const int64_t c = 16 * J + 4 * u + g;
        word |= (c < nchunk ? (unsigned)es[row * sstride + mx4_scale_slot(c, U)] : 127u) << (8 * u);
    }
    reinterpret_cast<unsigned *>(eo)[i] = word;
}
int launch_mx4_group_scales(Launcher &L, const uint8_t *e_stream, int64_t N, int64_t K, uint8_t *eo) {
    if (N <= 0 || K <= 0 || K % 32 || !e_stream || !eo) FL_FAIL(FL_ERR_BAD_ARGUMENT, "mx4_group_scales: bad shape or null argument");
    const int64_t n = N * (rows_w4_scale_stride(K) / 4);
    Launcher LL = L; LL.tag = "mx4_group_scales";
    return LL.launch(KC_CONVERT, (double)N * (mx4_scale_stride(K) + rows_w4_scale_stride(K)), 0.0, mx4_group_scales_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, e_stream, N, K,
                     mx4_u(K), mx4_scale_stride(K), eo);
}

}  // namespace fl
