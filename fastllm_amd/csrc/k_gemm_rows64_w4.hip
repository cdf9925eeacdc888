// k_gemm_rows64_w4.hip -- the 17-64-row weight stream over MXFP4 weights: Y[T,N] = rs[t] * (X[T,K] . W'[N,K]^T),
// W'[n,k] = 2^(e[n, k / 32] - 127) * q[n,k].
//
// The wide sibling of gemm_rows_w4_kernel (k_gemm_rows_w4.hip; same operands: the nibbles [N, K/2] and the group-order scale stream
// that launch_mx4_group_scales writes, same conversion) and the 4-bit sibling of gemm_rows64_w8_kernel (k_gemm_rows64_w8.hip), for the
// decode step of a batch of 17-64 streams on an FL_WEIGHTS_MXFP4 model under fl_tune "rows_w4".  The 2-16-row kernel keeps all rows of
// x in LDS for a whole K slice and has ONE token tile: a converted operand feeds one MFMA.  Here:
//   - x goes through LDS in K blocks of 512 columns -- one scale group, four wave instructions -- [T][512 + 8] bf16, double buffered.
//     The four waves of a workgroup walk the blocks together: while block i is consumed, every thread holds its 16-byte pieces of
//     block i + 1 in registers (requested before the weights of the same item: loads return in order, the LDS store must not wait for
//     the weight stream) and stores them behind the MFMAs; one barrier per block.  Columns past the end of the slice are stored as
//     zeros, rows past T are neither stored nor needed (a lane of such a row reads row T - 1; an A row of an MFMA reaches its own C
//     row only, which the epilogue does not store).  The row stride, 65 x 16 bytes, is odd in 16-byte units: the 16 rows x one column
//     of a ds_read_b128 cover all 64 banks once.
//     512 rather than 256 columns: an item is then exactly one scale dword per lane and tile, half the barriers, and 8 KB of weights
//     per wave.  The price is LDS: 2 x T x 1040 bytes, 65 KB at 32 rows (two workgroups to a CU up to 39 rows) and 130 KB at 64 rows
//     (one).  One is what the registers allow there anyway: 4 x 2 accumulators, three weight buffers and 16 x pieces are past 256
//     VGPRs, i.e. one wave per SIMD.
//   - weights never touch LDS.  A wave owns a row group of 32 weight rows -- two 16-row tiles; for gate/up the gate | up pair of the
//     16-interleaved layout; 16 rows where 32 would leave CUs without a workgroup -- and lane (r = lane & 15, g = lane >> 4) loads 16
//     bytes = one MX block, block 16 J + 4 u + g of row n0 + 16 j + r for instruction u of group J, non-temporal, straight to VGPRs,
//     and ONE dword of the group-order scale stream per tile: the scales of its four blocks.  The wave's (row group, K block) items
//     form one load stream, TWO items ahead in three register buffers (16 KB per wave in flight with two tiles); every load is
//     unconditional (counted vmcnt waits): a row past N re-reads row N - 1, a block past the end of K the last block (its x is zero,
//     its scale slot holds 2^0), and behind the last item the stream re-reads the last group.
//   - reuse.  A dword (8 nibbles) goes through four v_cvt_scalef32_pk_bf16_fp4 with the lane's block scale (byte << 23) ONCE and is
//     the B operand of ceil(T / 16) v_mfma_f32_16x16x32_bf16, one per token tile -- tokens are the A rows, the 16 weight rows the B
//     columns -- against one in the 2-16-row kernel: 16 converts per 16 x NTT MFMAs.  The x fragment of MFMA d of instruction u for
//     lane (t, g) is x[t][128 u + 32 g + 8 d .. + 7], the K permutation of k_gemm_rows_w4.hip; a fragment (four ds_read_b128, 64
//     contiguous bytes of the lane's x row) feeds both tiles of the row group.  NTT x NT fp32 16 x 16 accumulators.
//   - K slices over blockIdx.y (multiples of 512 columns: whole scale groups) for the narrow matrices, fp32 slabs [nks][T][N] that the
//     launch behind sums in slab order; EPI_F32 only, and only where the caller takes slabs (gemm_rows64_w4_plan).
//   - epilogues: EPI_F32 acc * rs[t]; EPI_GATEUP silu(g) * u as bf16 with the index map of the other row kernels.  No bias, no row
//     scale of the weights.  The rows equal the bf16-image rows up to fp32 summation order.
// K must be a multiple of 32 (a lane's load, one block).
#include <stdlib.h>

#include <algorithm>

#include "gemv_geometry.h"
#include "kernels.h"

namespace fl {

constexpr int kRows64W4Waves = 4;                       // waves of a workgroup: one per SIMD
constexpr int kRows64W4Threads = 64 * kRows64W4Waves;
constexpr int kRows64W4KB = kRowsW4Group;               // columns of a K block: one scale group, four instructions
constexpr int kRows64W4Stride = kRows64W4KB + 8;        // bf16 elements of an LDS row: 65 x 16 bytes

struct Rows64W4Args {
    const uint8_t *q, *e;                               // [N, K/2] nibbles; the group-order scale stream, `es` bytes per row
    const bf16_t *x;                                    // [T,K]
    const float *rs;                                    // [T], or null
    void *out;                                          // EPI_F32: float [nks][T][N]; EPI_GATEUP: bf16 [T][N/2]
    int T, N, K, Ks, es;                                // Ks: columns per slice (K, or a multiple of 512)
};

// NTT: 16-row token tiles, ceil(T / 16); NT: 16-row weight tiles of a wave's row group (gate | up: 2)
template <int NTT, int NT, int EPI>
__global__ __launch_bounds__(kRows64W4Threads) void gemm_rows64_w4_kernel(const Rows64W4Args a) {
    constexpr int KB = kRows64W4KB, ST = kRows64W4Stride, nthr = kRows64W4Threads, nwv = kRows64W4Waves;
    constexpr int XP = NTT * 16 * (KB / 8) / nthr;                                  // 16-byte pieces of an x block per thread
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    bf16_t *xs = reinterpret_cast<bf16_t *>(lds_raw);                               // two buffers of [T][ST]
    const int T = a.T, N = a.N, K = a.K;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r16 = lane & 15, g = lane >> 4;
    const int k0 = blockIdx.y * a.Ks, Ksl = min(a.Ks, K - k0);                       // this workgroup's slice of K: a multiple of 32, k0 of 512
    const int nblk = Ksl >> 5;                                                      // MX blocks of a row's slice
    const int nb = (Ksl + KB - 1) / KB;                                             // K blocks = scale groups (the last may be partial)
    const int ngroups = (N + 16 * NT - 1) / (16 * NT);
    const int gw = blockIdx.x * nwv + wave, nw = gridDim.x * nwv;
    const int n_items = (ngroups + nw - 1) / nw * nb;                               // the same for every wave: they walk x together
    const int buf_elems = T * ST;

    struct Buf { uint4v w[NT][4]; unsigned e[NT]; };
    int lg = gw, lb = 0;                                                            // load stream: next item = (row group, block)
    auto load_next = [&](Buf &buf) {
        const int grp = min(lg, ngroups - 1);
#pragma unroll
        for (int j = 0; j < NT; j++) {
            const size_t row = (size_t)min(grp * 16 * NT + 16 * j + r16, N - 1);
            const uint8_t *wr = a.q + row * (size_t)(K >> 1) + (k0 >> 1);
#pragma unroll
            for (int u = 0; u < 4; u++)
                buf.w[j][u] = __builtin_nontemporal_load(reinterpret_cast<const uint4v *>(wr + (size_t)min(16 * lb + 4 * u + g, nblk - 1) * 16));
            buf.e[j] = __builtin_nontemporal_load(reinterpret_cast<const unsigned *>(a.e + row * (size_t)a.es + (size_t)(k0 / KB + lb) * 16 + 4 * g));
        }
        if (++lb == nb) { lb = 0; lg += nw; }
    };

    // x block `blk` of the slice: piece i of a thread is 8 columns of row i / 64; a row past T re-reads row T - 1 and is not stored,
    // columns past the end of the slice are zeros (a mask)
    uint4v xr[XP];
    auto x_request = [&](int blk) {
#pragma unroll
        for (int j = 0; j < XP; j++) {
            const int i = tid + j * nthr;
            const int t = min(i / (KB / 8), T - 1), c = blk * KB + (i % (KB / 8)) * 8;
            xr[j] = *reinterpret_cast<const uint4v *>(a.x + (size_t)t * K + k0 + min(c, Ksl - 8));
        }
    };
    auto x_store = [&](bf16_t *dst, int blk) {                                      // (the mask here: nothing waits for the loads before)
#pragma unroll
        for (int j = 0; j < XP; j++) {
            const int i = tid + j * nthr;
            const unsigned keep = blk * KB + (i % (KB / 8)) * 8 < Ksl ? ~0u : 0u;
            if (i / (KB / 8) < T) *reinterpret_cast<uint4v *>(dst + (i / (KB / 8)) * ST + (i % (KB / 8)) * 8) = xr[j] & keep;
        }
    };

    // three register buffers: the weights of an item are requested two items ahead; inside an item the x pieces go first
    Buf b0, b1, b2;
    x_request(0);
    load_next(b0);
    load_next(b1);
    x_store(xs, 0);
    __syncthreads();

    // this lane's row of every token tile, at its 64 bytes of an instruction
    int xoff[NTT];
#pragma unroll
    for (int tt = 0; tt < NTT; tt++) xoff[tt] = min(16 * tt + r16, T - 1) * ST + 32 * g;

    float4v acc[NTT][NT];
#pragma unroll
    for (int tt = 0; tt < NTT; tt++)
#pragma unroll
        for (int j = 0; j < NT; j++) acc[tt][j] = float4v{0.f, 0.f, 0.f, 0.f};

    auto finish_group = [&](int grp) {
        if (grp < ngroups) {
#pragma unroll
            for (int tt = 0; tt < NTT; tt++) {
#pragma unroll
                for (int rg = 0; rg < 4; rg++) {
                    const int m = 16 * tt + 4 * g + rg;
                    if (m >= T) continue;
                    const float rsv = a.rs ? a.rs[m] : 1.0f;
                    if constexpr (EPI == EPI_GATEUP) {
                        const int n = grp * 32 + r16;                               // the gate row; up = n + 16
                        const int qq = (n >> 5) * 16 + (n & 15);
                        const float gt = acc[tt][0][rg] * rsv, up = acc[tt][NT - 1][rg] * rsv;
                        reinterpret_cast<bf16_t *>(a.out)[(size_t)m * (N / 2) + qq] = float_to_bf16_bits(gt / (1.0f + expf(-gt)) * up);
                    } else {
#pragma unroll
                        for (int j = 0; j < NT; j++) {
                            const int n = grp * 16 * NT + 16 * j + r16;
                            if (n < N) reinterpret_cast<float *>(a.out)[((size_t)blockIdx.y * T + m) * N + n] = acc[tt][j][rg] * rsv;
                        }
                    }
                }
            }
        }
#pragma unroll
        for (int tt = 0; tt < NTT; tt++)
#pragma unroll
            for (int j = 0; j < NT; j++) acc[tt][j] = float4v{0.f, 0.f, 0.f, 0.f};
    };

    int cg = gw, cb = 0, item = 0;                                                  // consume stream
    // one item: request the next item's x block and the weights two items ahead, consume this one, store the x block behind the MFMAs
    auto step = [&](const Buf &cur, Buf &ahead) {
        const bf16_t *xb = xs + (item & 1) * buf_elems;
        const int xblk = cb + 1 == nb ? 0 : cb + 1;
        x_request(xblk);
        load_next(ahead);
#pragma unroll
        for (int u = 0; u < 4; u++) {
            bf16x8q w[NT][4];                                                       // converted once, for every token tile
#pragma unroll
            for (int j = 0; j < NT; j++) {
                const float sc = __uint_as_float(((cur.e[j] >> (8 * u)) & 0xffu) << 23);
#pragma unroll
                for (int d = 0; d < 4; d++) w[j][d] = e2m1x8_to_bf16x8(cur.w[j][u][d], sc);
            }
#pragma unroll
            for (int tt = 0; tt < NTT; tt++) {
                const bf16_t *xp = xb + xoff[tt] + 128 * u;
                bf16x8q xf[4];
#pragma unroll
                for (int d = 0; d < 4; d++) xf[d] = *reinterpret_cast<const bf16x8q *>(xp + 8 * d);
#pragma unroll
                for (int d = 0; d < 4; d++)
#pragma unroll
                    for (int j = 0; j < NT; j++) acc[tt][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xf[d], w[j][d], acc[tt][j], 0, 0, 0);
            }
        }
        if (++cb == nb) { finish_group(cg); cb = 0; cg += nw; }
        x_store(xs + ((item + 1) & 1) * buf_elems, xblk);
        item++;
        __syncthreads();
    };
    int t = 0;
#pragma nounroll
    for (; t + 3 <= n_items; t += 3) {
        step(b0, b2);
        step(b1, b0);
        step(b2, b1);
    }
    if (t < n_items) step(b0, b2);
    if (t + 1 < n_items) step(b1, b0);
}

static size_t rows64_w4_lds(int64_t T) { return (size_t)2 * (size_t)T * kRows64W4Stride * 2; }

// the slices of a product (0: not served), the columns of one and the 16-row tiles of a wave's row group
static int rows64_w4_slices(int64_t T, int64_t N, int64_t K, int epi, int max_split, int64_t *Ks_out, int *nt_out) {
    if (T < 17 || T > 64 || N <= 0 || N > (1 << 24) || K < 32 || K % 32 || K > (1 << 24)) return 0;
    if (epi != EPI_F32 && epi != EPI_GATEUP) return 0;
    if (epi == EPI_GATEUP && N % 32) return 0;
    const int cap = (epi == EPI_F32 && max_split > 1) ? max_split : 1;              // slabs: the plain epilogue, when the caller sums them
    // few rows (QKV, o_proj, down_proj): slices until every CU has a workgroup of 16-row groups, as long as a slice keeps at least
    // two K blocks (1024 columns: the rule of both siblings)
    const int64_t waves = (int64_t)device_cu_count() * kRows64W4Waves, blocks = (K + kRows64W4KB - 1) / kRows64W4KB;
    int nks = 1;
    while (nks < cap && (N + 15) / 16 * nks < waves && blocks / (nks + 1) >= 2) nks++;
    const int64_t Ks = nks <= 1 ? K : ((K + nks - 1) / nks + kRows64W4KB - 1) / kRows64W4KB * kRows64W4KB;
    nks = (int)((K + Ks - 1) / Ks);
    if (Ks_out) *Ks_out = Ks;
    // two tiles per wave (an x fragment read once for both) where that still gives every CU its four waves; gate | up always
    if (nt_out) *nt_out = (epi == EPI_GATEUP || (N + 31) / 32 * nks >= waves) ? 2 : 1;
    return nks;
}
int gemm_rows64_w4_plan(int64_t T, int64_t N, int64_t K, int epi, int max_split) { return rows64_w4_slices(T, N, K, epi, max_split, nullptr, nullptr); }

template <int NTT, int NT, int EPI>
static int launch_rows64_w4_te(Launcher &L, const Rows64W4Args &a, int nks) {
    auto kern = gemm_rows64_w4_kernel<NTT, NT, EPI>;
    const size_t lds = rows64_w4_lds(a.T);
    FL_TRY(raise_dynamic_lds(reinterpret_cast<const void *>(kern), lds));
    // row groups over waves by the rule of the decode streams (gemv_geometry.h), per slice, in workgroups of four waves
    const GemvGeometry geo = gemv_geometry(((int64_t)a.N + 16 * NT - 1) / (16 * NT), lds, device_cu_count(), 0, 0);
    const int wgs = (geo.blocks * geo.waves + kRows64W4Waves - 1) / kRows64W4Waves;
    char tag[40];
    snprintf(tag, sizeof tag, "rows%d,%dx%d%s,w4", a.T, a.N, a.K, EPI == EPI_GATEUP ? ",glu" : (nks > 1 ? ",splitK" : ""));
    Launcher LL = L; LL.tag = tag;
    return LL.launch(KC_GEMM_MFMA, (double)a.N * (a.K / 2 + a.es) + 2.0 * a.T * a.K, 2.0 * a.T * a.N * a.K, kern, dim3((unsigned)wgs, (unsigned)nks),
                     dim3(kRows64W4Threads), lds, a);
}

template <int NT, int EPI>
static int launch_rows64_w4_e(Launcher &L, const Rows64W4Args &a, int nks) {
    switch ((a.T + 15) / 16) {
    case 2: return launch_rows64_w4_te<2, NT, EPI>(L, a, nks);
    case 3: return launch_rows64_w4_te<3, NT, EPI>(L, a, nks);
    default: return launch_rows64_w4_te<4, NT, EPI>(L, a, nks);
    }
}

int launch_gemm_rows64_w4(Launcher &L, const uint8_t *q, const uint8_t *e, const void *x, void *y, int64_t T, int64_t N, int64_t K, int epi,
                          const float *row_scale, int max_split, int *n_split_out) {
    if (n_split_out) *n_split_out = 1;
    if (!q || !e || !x || !y) FL_FAIL(FL_ERR_BAD_ARGUMENT, "launch_gemm_rows64_w4: null argument");
    int64_t Ks = 0;
    int nt = 2;
    const int nks = rows64_w4_slices(T, N, K, epi, n_split_out ? max_split : 1, &Ks, &nt);
    if (!nks) FL_FAIL(FL_ERR_UNSUPPORTED, "launch_gemm_rows64_w4: %lld x %lld x %lld (epilogue %d) is not served: 17..64 rows, K a multiple of 32, gate/up rows a multiple of 32", (long long)T, (long long)N, (long long)K, epi);
    FL_TRY(rs_parts_to_vector(L, row_scale, T));       // (a residual epilogue may have left 1/rms as partial sums)
    if (n_split_out) *n_split_out = nks;
    Rows64W4Args a;
    a.q = q; a.e = e; a.x = reinterpret_cast<const bf16_t *>(x); a.rs = row_scale; a.out = y;
    a.T = (int)T; a.N = (int)N; a.K = (int)K; a.Ks = (int)Ks; a.es = (int)rows_w4_scale_stride(K);
    if (epi == EPI_GATEUP) return launch_rows64_w4_e<2, EPI_GATEUP>(L, a, nks);
    return nt == 2 ? launch_rows64_w4_e<2, EPI_F32>(L, a, nks) : launch_rows64_w4_e<1, EPI_F32>(L, a, nks);
}

}  // namespace fl
