// k_gemm_rows128_w4.hip -- the 65-128-row weight stream over MXFP4 weights: Y[T,N] = rs[t] * (X[T,K] . W'[N,K]^T),
// W'[n,k] = 2^(e[n, k / 32] - 127) * q[n,k].
//
// The tall sibling of gemm_rows64_w4_kernel (k_gemm_rows64_w4.hip; same operands: the nibbles [N, K/2] and the group-order scale
// stream that launch_mx4_group_scales writes, same conversion, same epilogues), for the packed forwards of 65-128 rows on an
// FL_WEIGHTS_MXFP4 model under fl_tune "rows_w4".  The 64-row design keeps two 512-column blocks of x in LDS (130 KB at 64 rows) and
// 4 x 2 accumulators beside three 8-KB weight buffers per wave (282-374 VGPRs): neither doubles.  Here:
//   - x goes through LDS in STAGES of 128 columns, [T][128 + 8] bf16, double buffered: 2 x T x 272 bytes, 69.6 KB at 128 rows (the
//     registers, not LDS, keep it at one workgroup per CU: below).  The row stride, 17 x 16 bytes, is odd in 16-byte units:
//     the 16 rows x one column of a ds_read_b128 cover all 64 banks once.  The four waves of a workgroup walk the stages together:
//     while stage i is consumed every thread holds its ceil(T / 16) 16-byte pieces of stage i + 1 in registers and stores them
//     behind the MFMAs; one barrier per stage.  The pieces of BOTH stages behind a pair's first are requested there, before the
//     weights of the same step: loads return in order, the LDS store must not wait for the weight stream.  Columns past the end of
//     the slice are stored as zeros, rows past T are neither stored nor
//     needed (a lane of such a row reads row T - 1; an A row of an MFMA reaches its own C row only, which the epilogue does not store).
//   - a stage is not 128 ADJACENT columns.  Two stages make a PAIR of 256 columns = 8 MX blocks, and stage h of pair P holds the
//     columns of the blocks 8 P + 2 g + h, g = 0..3, at LDS columns 32 g ..: lane (r = lane & 15, g = lane >> 4) then owns the two
//     ADJACENT blocks 8 P + 2 g and 8 P + 2 g + 1 of its weight row -- 32 contiguous bytes, the four g of a row 128: a wave's weight
//     request covers whole 128-byte lines, each exactly once per launch (non-temporal), where 128 adjacent columns per stage would
//     ask for half a line now and the other half a stage later.  x pays for it with 64-byte runs in its global reads; x is small
//     and stays in L2.
//   - weights never touch LDS.  A wave owns a row group of 32 weight rows -- two 16-row tiles; for gate/up the gate | up pair of
//     the 16-interleaved layout; 16 rows where 32 would leave CUs without a workgroup -- and its (row group, pair) steps form one
//     load stream, TWO pairs ahead in three register buffers (8 KB per wave in flight with two tiles); every load is unconditional
//     (counted vmcnt waits): a row past N re-reads row N - 1, a block past the end of K the last block (its x is zero, its scale
//     slot holds 2^0), and behind the last step the stream re-reads the last group.  The two scales of a lane's blocks are two byte
//     loads from the group-order stream (cached: the 16 bytes of a scale group serve two pairs and four g).
//   - reuse.  A dword (8 nibbles) goes through four v_cvt_scalef32_pk_bf16_fp4 with the lane's block scale (byte << 23) ONCE and is
//     the B operand of ceil(T / 16) = 5..8 v_mfma_f32_16x16x32_bf16, one per token tile -- tokens are the A rows, the 16 weight
//     rows the B columns: 32 converts per 16 x NTT MFMAs with two tiles.  The x fragment of MFMA d for lane (t, g) is the 16 bytes at
//     LDS column 32 g + 8 d of row t; a fragment (four ds_read_b128, 64 contiguous bytes) feeds both tiles of the row group, so the
//     CU's LDS delivers one 1-KiB fragment per TWO MFMAs of a SIMD.  NTT x NT fp32 16 x 16 accumulators: 64 VGPRs at 128 rows.
//   - registers.  Accumulators, three weight buffers (60), the x pieces (2 x NTT x 4), the converted operands (32) and two fragments in
//     flight come to 476 registers with two tiles at eight token tiles (256 VGPRs + 220 AGPRs): one wave per SIMD, one workgroup per CU,
//     and the grid asks for no more.  Held to 256 (two waves per SIMD) the compiler spills 24-78 registers from six token tiles
//     on; Mistral-7B's widest matrices (896-1000 row groups of 32) have no second workgroup per CU to give anyway.
//   - K slices over blockIdx.y (multiples of 512 columns: whole scale groups and whole pairs) for the narrow matrices, fp32 slabs
//     [nks][T][N] that the launch behind sums in slab order; EPI_F32 only, and only where the caller takes slabs
//     (gemm_rows128_w4_plan).
//   - epilogues: EPI_F32 acc * rs[t]; EPI_GATEUP silu(g) * u as bf16 with the index map of the other row kernels.  No bias, no row
//     scale of the weights.  The rows equal the bf16-image rows up to fp32 summation order.
// K must be a multiple of 32 (a lane's load, one block).
#include <stdlib.h>

#include <algorithm>

#include "kernels.h"

namespace fl {

constexpr int kRows128W4Waves = 4;                      // waves of a workgroup: one per SIMD
constexpr int kRows128W4Threads = 64 * kRows128W4Waves;
constexpr int kRows128W4Stage = 128;                    // columns of an x stage: four MX blocks, one per lane group
constexpr int kRows128W4Pair = 2 * kRows128W4Stage;     // columns of a weight step: two adjacent blocks per lane
constexpr int kRows128W4Stride = kRows128W4Stage + 8;   // bf16 elements of an LDS row: 17 x 16 bytes

struct Rows128W4Args {
    const uint8_t *q, *e;                               // [N, K/2] nibbles; the group-order scale stream, `es` bytes per row
    const bf16_t *x;                                    // [T,K]
    const float *rs;                                    // [T], or null
    void *out;                                          // EPI_F32: float [nks][T][N]; EPI_GATEUP: bf16 [T][N/2]
    int T, N, K, Ks, es;                                // Ks: columns per slice (K, or a multiple of 512)
};

// NTT: 16-row token tiles, ceil(T / 16); NT: 16-row weight tiles of a wave's row group (gate | up: 2)
template <int NTT, int NT, int EPI>
__global__ __launch_bounds__(kRows128W4Threads) void gemm_rows128_w4_kernel(const Rows128W4Args a) {
    constexpr int ST = kRows128W4Stride, nwv = kRows128W4Waves;
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    bf16_t *xs = reinterpret_cast<bf16_t *>(lds_raw);                               // two buffers of [T][ST]
    const int T = a.T, N = a.N, K = a.K;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r16 = lane & 15, g = lane >> 4;
    const int k0 = blockIdx.y * a.Ks, Ksl = min(a.Ks, K - k0);                       // this workgroup's slice of K: a multiple of 32, k0 of 512
    const int nblk = Ksl >> 5;                                                      // MX blocks of a row's slice
    const int np = (Ksl + kRows128W4Pair - 1) / kRows128W4Pair;                     // pairs of the slice (the last may be partial)
    const int ngroups = (N + 16 * NT - 1) / (16 * NT);
    const int gw = blockIdx.x * nwv + wave, nw = gridDim.x * nwv;
    const int n_steps = (ngroups + nw - 1) / nw * np;                               // the same for every wave: they walk x together
    const int buf_elems = T * ST;

    // a step's weights: the lane's two adjacent blocks of every tile and their scales
    struct Buf { uint4v w[NT][2]; unsigned e[NT][2]; };
    int lg = gw, lp = 0;                                                            // load stream: next step = (row group, pair)
    auto load_next = [&](Buf &buf) {
        const int grp = min(lg, ngroups - 1);
        // block 8 P + 2 g + h is block 4 u + g' of its scale group with u = 2 (P & 1) + (g >> 1), g' = 2 (g & 1) + h: byte 4 g' + u
        const size_t eoff = (size_t)((k0 >> 9) + (lp >> 1)) * 16 + 8 * (g & 1) + 2 * (lp & 1) + (g >> 1);
#pragma unroll
        for (int j = 0; j < NT; j++) {
            const size_t row = (size_t)min(grp * 16 * NT + 16 * j + r16, N - 1);
            const uint8_t *wr = a.q + row * (size_t)(K >> 1) + (k0 >> 1);
            const uint8_t *er = a.e + row * (size_t)a.es + eoff;
#pragma unroll
            for (int h = 0; h < 2; h++) {
                buf.w[j][h] = __builtin_nontemporal_load(reinterpret_cast<const uint4v *>(wr + (size_t)min(8 * lp + 2 * g + h, nblk - 1) * 16));
                buf.e[j][h] = er[4 * h];
            }
        }
        if (++lp == np) { lp = 0; lg += nw; }
    };

    // x stage s = 2 P + h of the slice: a thread's piece j is 8 columns of row tid / 16 + 16 j, the same 8 columns in every piece --
    // LDS columns 8 (tid & 15), i.e. columns 8 (tid & 3) of block 8 P + 2 ((tid & 15) >> 2) + h.  A row past T re-reads row T - 1 and
    // is not stored, columns past the end of the slice are zeros (a mask)
    const int xrow = tid >> 4, xcol = (tid & 15) * 8, xsrc = 64 * ((tid & 15) >> 2) + 8 * (tid & 3);
    auto stage_col = [&](int s) { return (s >> 1) * kRows128W4Pair + (s & 1) * 32 + xsrc; };
    uint4v xr[2][NTT];
    auto x_request = [&](uint4v *xq, int s) {
        const bf16_t *src = a.x + k0 + min(stage_col(s), Ksl - 8);
#pragma unroll
        for (int j = 0; j < NTT; j++) xq[j] = *reinterpret_cast<const uint4v *>(src + (size_t)min(xrow + 16 * j, T - 1) * K);
    };
    auto x_store = [&](bf16_t *dst, const uint4v *xq, int s) {                      // (the mask here: nothing waits for the loads before)
        const unsigned keep = stage_col(s) < Ksl ? ~0u : 0u;
#pragma unroll
        for (int j = 0; j < NTT; j++)
            if (xrow + 16 * j < T) *reinterpret_cast<uint4v *>(dst + (xrow + 16 * j) * ST + xcol) = xq[j] & keep;
    };

    // three register buffers: the weights of a step are requested two steps ahead; inside a step the x pieces go first
    Buf b0, b1, b2;
    x_request(xr[0], 0);
    load_next(b0);
    load_next(b1);
    x_store(xs, xr[0], 0);
    __syncthreads();

    // this lane's row of every token tile, at its 64 bytes of a stage
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

    int cg = gw, cp = 0, item = 0;                                                  // consume stream; item: stages done
    // one step = the two stages of a pair.  Per stage: request the next stage of x (and, in the first, the weights two steps ahead),
    // consume this one, store the next stage behind the MFMAs
    auto step = [&](const Buf &cur, Buf &ahead) {
#pragma unroll
        for (int h = 0; h < 2; h++) {
            const bf16_t *xb = xs + (item & 1) * buf_elems;
            // BOTH next stages of x are requested in the first stage, ahead of the step's weight request: loads return in order, and
            // an x request behind it would make its LDS store wait for weights that are not due for two steps
            const int ns = h == 0 ? 2 * cp + 1 : (cp + 1 == np ? 0 : 2 * cp + 2);   // (behind a group's last stage: the next group's first)
            if (h == 0) {
                x_request(xr[0], ns);
                x_request(xr[1], cp + 1 == np ? 0 : 2 * cp + 2);
                load_next(ahead);
            }
            bf16x8q w[NT][4];                                                       // converted once, for every token tile
#pragma unroll
            for (int j = 0; j < NT; j++) {
                const float sc = __uint_as_float(cur.e[j][h] << 23);
#pragma unroll
                for (int d = 0; d < 4; d++) w[j][d] = e2m1x8_to_bf16x8(cur.w[j][h][d], sc);
            }
            // the fragments of token tile tt + 1 are requested from LDS before the MFMAs of tile tt: with one wave per SIMD nothing
            // else covers the ds_read -> MFMA latency
            bf16x8q xf[2][4];
#pragma unroll
            for (int d = 0; d < 4; d++) xf[0][d] = *reinterpret_cast<const bf16x8q *>(xb + xoff[0] + 8 * d);
#pragma unroll
            for (int tt = 0; tt < NTT; tt++) {
                if (tt + 1 < NTT) {
#pragma unroll
                    for (int d = 0; d < 4; d++) xf[(tt + 1) & 1][d] = *reinterpret_cast<const bf16x8q *>(xb + xoff[tt + 1] + 8 * d);
                }
                __builtin_amdgcn_sched_barrier(0);                                   // (the scheduler would sink the reads to two MFMAs before their use)
#pragma unroll
                for (int d = 0; d < 4; d++)
#pragma unroll
                    for (int j = 0; j < NT; j++) acc[tt][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xf[tt & 1][d], w[j][d], acc[tt][j], 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
            }
            if (h == 1 && ++cp == np) { finish_group(cg); cp = 0; cg += nw; }
            x_store(xs + ((item + 1) & 1) * buf_elems, xr[h], ns);
            item++;
            __syncthreads();
        }
    };
    int t = 0;
#pragma nounroll
    for (; t + 3 <= n_steps; t += 3) {
        step(b0, b2);
        step(b1, b0);
        step(b2, b1);
    }
    if (t < n_steps) step(b0, b2);
    if (t + 1 < n_steps) step(b1, b0);
}

static size_t rows128_w4_lds(int64_t T) { return (size_t)2 * (size_t)T * kRows128W4Stride * 2; }

// the slices of a product (0: not served), the columns of one and the 16-row tiles of a wave's row group
static int rows128_w4_slices(int64_t T, int64_t N, int64_t K, int epi, int max_split, int64_t *Ks_out, int *nt_out) {
    if (T < 65 || T > 128 || N <= 0 || N > (1 << 24) || K < 32 || K % 32 || K > (1 << 24)) return 0;
    if (epi != EPI_F32 && epi != EPI_GATEUP) return 0;
    if (epi == EPI_GATEUP && N % 32) return 0;
    const int cap = (epi == EPI_F32 && max_split > 1) ? max_split : 1;              // slabs: the plain epilogue, when the caller sums them
    // few rows (QKV, o_proj, down_proj): slices until every CU has a workgroup of 16-row groups, as long as a slice keeps at least
    // two scale groups (1024 columns: the rule of the siblings)
    const int64_t waves = (int64_t)device_cu_count() * kRows128W4Waves, blocks = (K + kRowsW4Group - 1) / kRowsW4Group;
    int nks = 1;
    while (nks < cap && (N + 15) / 16 * nks < waves && blocks / (nks + 1) >= 2) nks++;
    const int64_t Ks = nks <= 1 ? K : ((K + nks - 1) / nks + kRowsW4Group - 1) / kRowsW4Group * kRowsW4Group;
    nks = (int)((K + Ks - 1) / Ks);
    if (Ks_out) *Ks_out = Ks;
    // two tiles per wave (an x fragment read once for both) where that still gives every CU its four waves; gate | up always
    if (nt_out) *nt_out = (epi == EPI_GATEUP || (N + 31) / 32 * nks >= waves) ? 2 : 1;
    return nks;
}
int gemm_rows128_w4_plan(int64_t T, int64_t N, int64_t K, int epi, int max_split) { return rows128_w4_slices(T, N, K, epi, max_split, nullptr, nullptr); }

template <int NTT, int NT, int EPI>
static int launch_rows128_w4_te(Launcher &L, const Rows128W4Args &a, int nks) {
    auto kern = gemm_rows128_w4_kernel<NTT, NT, EPI>;
    const size_t lds = rows128_w4_lds(a.T);
    FL_TRY(raise_dynamic_lds(reinterpret_cast<const void *>(kern), lds));
    // one row group per wave where the CUs have room for all of them at once (one workgroup to a CU: the registers); beyond that
    // as many rounds as it takes, over the fewest workgroups that still need only that many
    const int64_t ngroups = ((int64_t)a.N + 16 * NT - 1) / (16 * NT), need = (ngroups + kRows128W4Waves - 1) / kRows128W4Waves;
    const int64_t room = std::max<int64_t>(device_cu_count() / nks, 1);
    const int64_t rounds = (need + room - 1) / room;
    const int64_t wgs = (need + rounds - 1) / rounds;
    char tag[40];
    snprintf(tag, sizeof tag, "rows%d,%dx%d%s,w4", a.T, a.N, a.K, EPI == EPI_GATEUP ? ",glu" : (nks > 1 ? ",splitK" : ""));
    Launcher LL = L; LL.tag = tag;
    return LL.launch(KC_GEMM_MFMA, (double)a.N * (a.K / 2 + a.es) + 2.0 * a.T * a.K, 2.0 * a.T * a.N * a.K, kern, dim3((unsigned)wgs, (unsigned)nks),
                     dim3(kRows128W4Threads), lds, a);
}

template <int NT, int EPI>
static int launch_rows128_w4_e(Launcher &L, const Rows128W4Args &a, int nks) {
    switch ((a.T + 15) / 16) {
    case 5: return launch_rows128_w4_te<5, NT, EPI>(L, a, nks);
    case 6: return launch_rows128_w4_te<6, NT, EPI>(L, a, nks);
    case 7: return launch_rows128_w4_te<7, NT, EPI>(L, a, nks);
    default: return launch_rows128_w4_te<8, NT, EPI>(L, a, nks);
    }
}

int launch_gemm_rows128_w4(Launcher &L, const uint8_t *q, const uint8_t *e, const void *x, void *y, int64_t T, int64_t N, int64_t K, int epi,
                           const float *row_scale, int max_split, int *n_split_out) {
    if (n_split_out) *n_split_out = 1;
    if (!q || !e || !x || !y) FL_FAIL(FL_ERR_BAD_ARGUMENT, "launch_gemm_rows128_w4: null argument");
    int64_t Ks = 0;
    int nt = 2;
    const int nks = rows128_w4_slices(T, N, K, epi, n_split_out ? max_split : 1, &Ks, &nt);
    if (!nks) FL_FAIL(FL_ERR_UNSUPPORTED, "launch_gemm_rows128_w4: %lld x %lld x %lld (epilogue %d) is not served: 65..128 rows, K a multiple of 32, gate/up rows a multiple of 32", (long long)T, (long long)N, (long long)K, epi);
    FL_TRY(rs_parts_to_vector(L, row_scale, T));       // (a residual epilogue may have left 1/rms as partial sums)
    if (n_split_out) *n_split_out = nks;
    Rows128W4Args a;
    a.q = q; a.e = e; a.x = reinterpret_cast<const bf16_t *>(x); a.rs = row_scale; a.out = y;
    a.T = (int)T; a.N = (int)N; a.K = (int)K; a.Ks = (int)Ks; a.es = (int)rows_w4_scale_stride(K);
    if (epi == EPI_GATEUP) return launch_rows128_w4_e<2, EPI_GATEUP>(L, a, nks);
    return nt == 2 ? launch_rows128_w4_e<2, EPI_F32>(L, a, nks) : launch_rows128_w4_e<1, EPI_F32>(L, a, nks);
}

}  // namespace fl
