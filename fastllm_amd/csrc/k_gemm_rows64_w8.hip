// k_gemm_rows64_w8.hip -- the 17-64-row weight stream over FP8 weights: Y[T,N] = rs[t] * s[n] * (X[T,K] . q[N,K]^T).
//
// The wide sibling of gemm_rows_w8_kernel (k_gemm_rows_w8.hip; same format, same conversion, same guarantee), for the decode step of a
// batch of 17-64 streams on an FL_WEIGHTS_E4M3_ROW model.  That kernel keeps all T rows of x in LDS for a whole K slice -- T * (Ks + 8)
// * 2 bytes, and gate/up may not be sliced: at K = 4096 the 160 KB end at 19 rows.  Here x moves differently:
//   - x goes through LDS in K blocks of 256 columns, [T][256 + 8] bf16, double buffered (2 x 33 KB at 64 rows).  The four waves of a
//     workgroup walk the blocks together: while block i is consumed, every thread holds its 16-byte pieces of block i + 1 in
//     registers (global loads issued before the MFMAs) and stores them behind the MFMAs; one barrier per block.  Columns past the end
//     of the slice are stored as zeros, rows past T are never stored nor needed (a lane of such a row reads row T - 1; an A row of an
//     MFMA reaches its own C row only, which the epilogue does not store).  The row stride, 33 x 16 bytes, is odd in 16-byte units:
//     the 16 rows x one column of a ds_read_b128 are conflict-free.
//   - weights never touch LDS.  A wave owns a row group of 32 weight rows -- two 16-row tiles; for gate/up the gate | up pair of the
//     16-interleaved layout; 16 rows where 32 would leave CUs without a workgroup -- and lane (r = lane & 15, g = lane >> 4) loads 16
//     bytes of row n0 + 16 j + r at k0 + 64 u + 16 g, non-temporal, straight to VGPRs: 2 x 4 loads per block, TWO blocks ahead in
//     three register buffers (16 KB per wave in flight).  The wave's (row group, K block) items form one load stream; every load is
//     unconditional (counted vmcnt waits): a row past N re-reads row N - 1, a chunk past the end of K the last chunk (its x is
//     zero), and behind the last item the stream re-reads the last group.  The x pieces of an item are requested before its weights:
//     loads return in order, and the LDS store must not wait for the weight stream (it did at first: 1.8 instead of 2.8 TB/s).
//   - reuse.  A loaded 16 bytes are converted once (v_cvt_scalef32_pk_bf16_fp8, scale 1.0: exact; two 8-element operands) and feed
//     2 * ceil(T / 16) v_mfma_f32_16x16x32_bf16 -- tokens are the A rows, the 16 weight rows the B columns -- against 2 in the 16-row
//     kernel.  An x fragment (two ds_read_b128) feeds both tiles of the row group: 4 MFMAs per 32 bytes read from LDS, i.e. 4 bytes of
//     ds_read per weight byte at 64 rows (8 with one tile per wave, as much as the LDS pipe has beside the HBM stream).
//     ceil(T / 16) x 2 fp32 16 x 16 accumulators: 32 VGPRs at 64 rows.  No VALU work in the loop but the conversion.
//   - K slices over blockIdx.y (multiples of 256 columns) for the narrow matrices, fp32 slabs [nks][T][N] that the rmsnorm_add /
//     rope_kv launch behind sums in slab order; EPI_F32 only, and only where the caller takes slabs (gemm_rows64_w8_plan).
//   - epilogues: EPI_F32 acc * s[n] * rs[t]; EPI_GATEUP silu(g) * u as bf16 with the index map of gemm_rows_w8_kernel.  No bias.
//     s is a power of two: acc * s is exact, the rows equal the bf16-image rows up to fp32 summation order.
// K must be a multiple of 16 (a lane's load).
#include <stdlib.h>

#include <algorithm>

#include "gemv_geometry.h"
#include "kernels.h"

namespace fl {

constexpr int kRows64Waves = 4;                     // waves of a workgroup: one per SIMD, up to 512 VGPRs each
constexpr int kRows64Threads = 64 * kRows64Waves;
constexpr int kRows64U = 4;                         // 64-column MFMA steps of a K block
constexpr int kRows64KB = 64 * kRows64U;            // columns of a K block
constexpr int kRows64Stride = kRows64KB + 8;        // bf16 elements of an LDS row: 33 x 16 bytes
typedef __bf16 bf16x8r __attribute__((ext_vector_type(8)));

struct Rows64W8Args {
    const uint8_t *q; const float *s;               // [N,K] e4m3, [N]
    const bf16_t *x;                                // [T,K]
    const float *rs;                                // [T], or null
    void *out;                                      // EPI_F32: float [nks][T][N]; EPI_GATEUP: bf16 [T][N/2]
    int T, N, K, Ks;                                // Ks: columns per slice (a multiple of 256, or >= K)
};

__device__ inline bf16x8r rows64_e4m3x8(unsigned lo, unsigned hi) {   // as e4m3x8_to_bf16x8: element i = byte i
    uint4v r;
    r[0] = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(lo, 1.0f, false));
    r[1] = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(lo, 1.0f, true));
    r[2] = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(hi, 1.0f, false));
    r[3] = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(hi, 1.0f, true));
    return __builtin_bit_cast(bf16x8r, r);
}

// NTT: 16-row token tiles, ceil(T / 16); NT: 16-row weight tiles of a wave's row group (gate | up: 2)
template <int NTT, int NT, int EPI>
__global__ __launch_bounds__(kRows64Threads) void gemm_rows64_w8_kernel(const Rows64W8Args a) {
    constexpr int U = kRows64U, KB = kRows64KB, ST = kRows64Stride, nthr = kRows64Threads, nwv = kRows64Waves;
    constexpr int XP = NTT * 16 * (KB / 8) / nthr;                                  // 16-byte pieces of an x block per thread
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    bf16_t *xs = reinterpret_cast<bf16_t *>(lds_raw);                               // two buffers of [T][ST]
    const int T = a.T, N = a.N, K = a.K;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r16 = lane & 15, g = lane >> 4;
    const int k0 = blockIdx.y * a.Ks, Ksl = min(a.Ks, K - k0);                       // this workgroup's slice of K: a multiple of 16
    const int nchunk = Ksl >> 4;                                                    // 16-weight chunks of a row's slice
    const int nb = (Ksl + KB - 1) / KB;                                             // K blocks (the last may be partial)
    const int ngroups = (N + 16 * NT - 1) / (16 * NT);
    const int gw = blockIdx.x * nwv + wave, nw = gridDim.x * nwv;
    const int n_items = (ngroups + nw - 1) / nw * nb;                               // the same for every wave: they walk x together
    const int buf_elems = T * ST;

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

    // x block `blk` of the slice: piece i of a thread is 8 columns of row i / 32; a row past T re-reads row T - 1 and is not stored,
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

    // three register buffers: the weights of an item are requested two items ahead.  Inside an item the x pieces are requested
    // BEFORE the weights: loads return in order, so the store of the x pieces then waits for them alone (vmcnt = the weight loads
    // behind them), not for the weight stream
    Buf b0, b1, b2;
    x_request(0);
    load_next(b0);
    load_next(b1);
    x_store(xs, 0);
    __syncthreads();

    // this lane's row of every token tile
    int xoff[NTT];
#pragma unroll
    for (int tt = 0; tt < NTT; tt++) xoff[tt] = min(16 * tt + r16, T - 1) * ST + 16 * g;

    float wsc[NT];
    auto group_prefetch = [&](int grp) {
#pragma unroll
        for (int j = 0; j < NT; j++) {
            const int n = grp * 16 * NT + 16 * j + r16;
            wsc[j] = n < N ? a.s[n] : 0.f;
        }
    };
    group_prefetch(min(gw, ngroups - 1));

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
                        const float gt = acc[tt][0][rg] * wsc[0] * rsv, up = acc[tt][NT - 1][rg] * wsc[NT - 1] * rsv;
                        reinterpret_cast<bf16_t *>(a.out)[(size_t)m * (N / 2) + qq] = float_to_bf16_bits(gt / (1.0f + expf(-gt)) * up);
                    } else {
#pragma unroll
                        for (int j = 0; j < NT; j++) {
                            const int n = grp * 16 * NT + 16 * j + r16;
                            if (n < N) reinterpret_cast<float *>(a.out)[((size_t)blockIdx.y * T + m) * N + n] = acc[tt][j][rg] * wsc[j] * rsv;
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
        if (cb == 0 && cg != gw) group_prefetch(min(cg, ngroups - 1));
#pragma unroll
        for (int u = 0; u < U; u++) {
            bf16x8r w[NT][2];
#pragma unroll
            for (int j = 0; j < NT; j++) {
                w[j][0] = rows64_e4m3x8(cur[j][u][0], cur[j][u][1]);
                w[j][1] = rows64_e4m3x8(cur[j][u][2], cur[j][u][3]);
            }
#pragma unroll
            for (int tt = 0; tt < NTT; tt++) {
                const bf16_t *xp = xb + xoff[tt] + 64 * u;
                const bf16x8r xa = *reinterpret_cast<const bf16x8r *>(xp), xc = *reinterpret_cast<const bf16x8r *>(xp + 8);
#pragma unroll
                for (int j = 0; j < NT; j++) {
                    acc[tt][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xa, w[j][0], acc[tt][j], 0, 0, 0);
                    acc[tt][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xc, w[j][1], acc[tt][j], 0, 0, 0);
                }
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

static size_t rows64_w8_lds(int64_t T) { return (size_t)2 * (size_t)T * kRows64Stride * 2; }

// the slices of a product (0: not served), the columns of one and the 16-row tiles of a wave's row group
static int rows64_w8_slices(int64_t T, int64_t N, int64_t K, int epi, int max_split, int64_t *Ks_out, int *nt_out) {
    if (T < 17 || T > 64 || N <= 0 || N > (1 << 24) || K < 16 || K % 16 || K > (1 << 24)) return 0;
    if (epi != EPI_F32 && epi != EPI_GATEUP) return 0;
    if (epi == EPI_GATEUP && N % 32) return 0;
    const int cap = (epi == EPI_F32 && max_split > 1) ? max_split : 1;              // slabs: the plain epilogue, when the caller sums them
    // few rows (QKV, o_proj, down_proj): slices until every CU has a workgroup of 16-row groups, as long as a slice keeps at least
    // four K blocks
    const int64_t waves = (int64_t)device_cu_count() * kRows64Waves, blocks = (K + kRows64KB - 1) / kRows64KB;
    int nks = 1;
    while (nks < cap && (N + 15) / 16 * nks < waves && blocks / (nks + 1) >= 4) nks++;
    const int64_t Ks = nks <= 1 ? K : ((K + nks - 1) / nks + kRows64KB - 1) / kRows64KB * kRows64KB;
    nks = (int)((K + Ks - 1) / Ks);
    if (Ks_out) *Ks_out = Ks;
    // two tiles per wave (an x fragment read once for both) where that still gives every CU its four waves; gate | up always
    if (nt_out) *nt_out = (epi == EPI_GATEUP || (N + 31) / 32 * nks >= waves) ? 2 : 1;
    return nks;
}
int gemm_rows64_w8_plan(int64_t T, int64_t N, int64_t K, int epi, int max_split) { return rows64_w8_slices(T, N, K, epi, max_split, nullptr, nullptr); }

template <int NTT, int NT, int EPI>
static int launch_rows64_w8_te(Launcher &L, const Rows64W8Args &a, int nks) {
    auto kern = gemm_rows64_w8_kernel<NTT, NT, EPI>;
    const size_t lds = rows64_w8_lds(a.T);
    FL_TRY(raise_dynamic_lds(reinterpret_cast<const void *>(kern), lds));
    // row groups over waves by the rule of the decode streams (gemv_geometry.h), per slice, in workgroups of four waves
    const GemvGeometry geo = gemv_geometry(((int64_t)a.N + 16 * NT - 1) / (16 * NT), lds, device_cu_count(), 0, 0);
    const int wgs = (geo.blocks * geo.waves + kRows64Waves - 1) / kRows64Waves;
    char tag[40];
    snprintf(tag, sizeof tag, "rows%d,%dx%d%s,w8", a.T, a.N, a.K, EPI == EPI_GATEUP ? ",glu" : (nks > 1 ? ",splitK" : ""));
    Launcher LL = L; LL.tag = tag;
    return LL.launch(KC_GEMM_MFMA, (double)a.N * a.K + 4.0 * a.N + 2.0 * a.T * a.K, 2.0 * a.T * a.N * a.K, kern, dim3((unsigned)wgs, (unsigned)nks),
                     dim3(kRows64Threads), lds, a);
}

template <int NT, int EPI>
static int launch_rows64_w8_e(Launcher &L, const Rows64W8Args &a, int nks) {
    switch ((a.T + 15) / 16) {
    case 2: return launch_rows64_w8_te<2, NT, EPI>(L, a, nks);
    case 3: return launch_rows64_w8_te<3, NT, EPI>(L, a, nks);
    default: return launch_rows64_w8_te<4, NT, EPI>(L, a, nks);
    }
}

int launch_gemm_rows64_w8(Launcher &L, const uint8_t *q, const float *s, const void *x, void *y, int64_t T, int64_t N, int64_t K, int epi,
                          const float *row_scale, int max_split, int *n_split_out) {
    if (n_split_out) *n_split_out = 1;
    if (!q || !s || !x || !y) FL_FAIL(FL_ERR_BAD_ARGUMENT, "launch_gemm_rows64_w8: null argument");
    int64_t Ks = 0;
    int nt = 2;
    const int nks = rows64_w8_slices(T, N, K, epi, n_split_out ? max_split : 1, &Ks, &nt);
    if (!nks) FL_FAIL(FL_ERR_UNSUPPORTED, "launch_gemm_rows64_w8: %lld x %lld x %lld (epilogue %d) is not served: 17..64 rows, K a multiple of 16, gate/up rows a multiple of 32", (long long)T, (long long)N, (long long)K, epi);
    FL_TRY(rs_parts_to_vector(L, row_scale, T));       // (a residual epilogue may have left 1/rms as partial sums)
    if (n_split_out) *n_split_out = nks;
    Rows64W8Args a;
    a.q = q; a.s = s; a.x = reinterpret_cast<const bf16_t *>(x); a.rs = row_scale; a.out = y;
    a.T = (int)T; a.N = (int)N; a.K = (int)K; a.Ks = (int)Ks;
    if (epi == EPI_GATEUP) return launch_rows64_w8_e<2, EPI_GATEUP>(L, a, nks);
    return nt == 2 ? launch_rows64_w8_e<2, EPI_F32>(L, a, nks) : launch_rows64_w8_e<1, EPI_F32>(L, a, nks);
}

}  // namespace fl
