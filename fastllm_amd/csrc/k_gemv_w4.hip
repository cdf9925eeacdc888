// k_gemv_w4.hip -- the decode (T = 1) weight stream over MXFP4 weights, and the quantiser that makes them.
//
// Format (FL_WEIGHTS_MXFP4): W'[n,k] = 2^e[n, k / 32] * q[n,k], q OCP e2m1 (grid 0, 0.5, 1, 1.5, 2, 3, 4, 6 and a sign bit), one
// e8m0 scale byte e + 127 per block of 32 consecutive k of a row; e is the smallest integer with absmax(block) / 2^e <= 6, kept
// at -120 or above (an all-zero block: e = 0), q = RNE(W / 2^e) with ties to the code whose mantissa bit is 0.  Byte j of a row
// holds element 2j in its low nibble and element 2j + 1 in its high nibble.  2^e * q is exact in bf16: an MXFP4 model is the
// bf16 model whose weights are W'.  4.25 bits per weight.
//
// The kernel is the sibling of k_gemv_w8.hip: same GemvArgs, and the row map, norm prologue, epilogues and geometry rule are
// the ones of gemv_parts.h / gemv_geometry.h; the stream is its own.  What differs:
//   - a lane's 16-byte non-temporal load is 32 weights -- exactly one MX block -- so a wave instruction (1 KiB) covers 2048
//     columns of a row and K = 4096 is two instructions long.  A row group is therefore FOUR rows (kW4R) and an item is
//     (row group, K block of U = 2 or 1 instructions): 8 KiB per item at K = 4096, 4 KiB at K = 14336 (7 instructions: U = 1
//     pads nothing), what the FP8 stream keeps per item on the same shapes.  A second register buffer runs one item ahead;
//     every load is unconditional (counted vmcnt waits): past the end of K a lane re-reads the row's last chunk with its x
//     zeroed, a row past N re-reads row N - 1.
//   - the scales are a second stream of 1/16 the bytes, laid out in HBM in stream order,
//         [row][K block][lane][u]   bytes,   row stride = nb * 64 * U,   nb = ceil(K / 32 / (64 U)),
//     so that a lane gets the scales of all its chunks of (row, item) with ONE U-byte load, requested with the data of the
//     same item.  Slots past K / 32 hold 127 (2^0).  U follows from K alone (mx4_u), so the layout is a function of K:
//     mx4_scale_stride(K) bytes per row.  The quantiser writes this layout; launch_mx4_layout converts from the logical
//     [N][K / 32].
//   - conversion: v_cvt_scalef32_pk_bf16_fp4 turns one byte (two e2m1) into a packed bf16 pair and applies the block's scale
//     -- the fp32 whose exponent field is the e8m0 byte, byte << 23 -- inside the instruction; the pair goes into
//     v_dot2c_f32_bf16 against the bf16 x of LDS (common.h: dot2c_bf16 / dot2c_settle carry the dot-result hazard wait).
//     16 converts + 16 dots per 32 weights, one VALU instruction per weight-lane.
//   - x in LDS is four planes (elements 0-7 | 8-15 | 16-23 | 24-31 of every 32-element chunk), so that each of a lane's
//     four ds_read_b128 is 16-byte strided across the wave.
//   - there is no per-row scale in the epilogue: 1/rms multiplies the reduced sum as before.
// K must be a multiple of 32 (a lane's load, one block); fl_model_create_opts refuses other shapes in this mode.
#include <stdlib.h>

#include "gemv_geometry.h"
#include "gemv_parts.h"
#include "kernels.h"

namespace fl {

constexpr int kW4MaxThreads = 768;       // 12 waves: 170 VGPRs per lane
constexpr int kW4R = 4;

// (mx4_u, the chunks per item, and mx4_scale_slot, the place of a block's scale in the stream: kernels.h)
int64_t mx4_scale_stride(int64_t K) {
    const int64_t per = 64 * mx4_u(K);
    return ((K >> 5) + per - 1) / per * per;
}

// byte B of `w` (two e2m1: low nibble first) times the scale as a packed bf16 pair
template <int B> __device__ inline unsigned e2m1x2_to_bf16x2(unsigned w, float scale) {
    return __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, scale, B));
}

template <int U> struct W4Scales;
template <> struct W4Scales<1> { typedef uint8_t T; };
template <> struct W4Scales<2> { typedef uint16_t T; };

template <int R, int U, int PRO, int EPI>
__global__ __launch_bounds__(kW4MaxThreads) void gemv_w4_kernel(const GemvArgs a, const uint8_t *__restrict__ escale) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    __shared__ float red[kW4MaxThreads / 64];
    __shared__ float cv[kW4MaxThreads / 64];         // ArgMax candidates of the waves (GemvArgs::amax)
    __shared__ int ci[kW4MaxThreads / 64];
    typedef typename W4Scales<U>::T sc_t;
    bf16_t *xs = reinterpret_cast<bf16_t *>(lds_raw);
    const uint8_t *__restrict__ W = reinterpret_cast<const uint8_t *>(a.W);
    const int N = a.N, K = a.K;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nthr = blockDim.x, nwv = nthr >> 6;
    const int nchunk = K >> 5;                       // 32-weight chunks (a lane's load, one MX block); K % 32 == 0
    const int nch8 = K >> 3;                         // 8-element chunks of the activation staging
    const int poff = K >> 2;                         // xs: four planes of K / 4 elements
    const int half = a.d >> 1;
    const int ngroups = (N + R - 1) / R;
    const int wave_u = __builtin_amdgcn_readfirstlane(wave);
    const int gw = blockIdx.x * nwv + wave_u, nw = gridDim.x * nwv;

    auto row_of = [&](int g, int r) -> int { return gemv_row_of<EPI, R>(g, r, a.d, half); };
    auto xs_slot = [&](int c8) -> int { return (c8 & 3) * poff + (c8 >> 2) * 8; };

    struct Buf { uint4v w[R][U]; sc_t e[R]; };
    Buf pre;
    const int nb = (nchunk + 64 * U - 1) / (64 * U);                                // K blocks per row group (the last may be partial)
    const size_t estride = (size_t)nb * 64 * U;                                     // bytes of a row in the scale stream
    const int n_items = gw < ngroups ? (ngroups - gw + nw - 1) / nw * nb : 0;      // this wave's items
    int lg = gw, lb = 0;                                                            // load stream: next item = (row group, block)
    // every load is unconditional: past the end of K a lane re-reads the last chunk (its x is zeroed; its scale slot holds 2^0),
    // a row past N re-reads row N - 1
    auto load_next = [&](Buf &buf) {
        const int g = min(lg, ngroups - 1);
#pragma unroll
        for (int r = 0; r < R; r++) {
            const int row = row_of(g, r);
            const size_t rw = (size_t)(row < N ? row : N - 1);
            const uint8_t *wr = W + rw * (size_t)(K >> 1);
#pragma unroll
            for (int u = 0; u < U; u++)
                buf.w[r][u] = __builtin_nontemporal_load(reinterpret_cast<const uint4v *>(wr + (size_t)min(lane + 64 * (U * lb + u), nchunk - 1) * 16));
            buf.e[r] = __builtin_nontemporal_load(reinterpret_cast<const sc_t *>(escale + rw * estride + (size_t)(lb * 64 + lane) * U));
        }
        if (++lb == nb) { lb = 0; lg += nw; }
    };

    float inv_m = 1.0f;
    if constexpr (PRO == PRO_NORM) {
        // three chunks of 8 per thread (nthr * 3 * 8 >= K, host-checked); the weight stream starts behind the activation loads
        inv_m = gemv_norm_prologue<3, bf16_t>(a, xs, red, xs_slot, [&]() { load_next(pre); });
    } else {
        const bf16_t *__restrict__ x = reinterpret_cast<const bf16_t *>(a.x);
        constexpr int NXR = 4;
        uint4v xr[NXR];
#pragma unroll
        for (int i = 0; i < NXR; i++) {
            const int c = tid + nthr * i;
            if (c < nch8) xr[i] = *reinterpret_cast<const uint4v *>(x + c * 8);
        }
        if (a.x_scale) inv_m = *a.x_scale;
        load_next(pre);
#pragma unroll
        for (int i = 0; i < NXR; i++) {
            const int c = tid + nthr * i;
            if (c < nch8) *reinterpret_cast<uint4v *>(xs + xs_slot(c)) = xr[i];
        }
        for (int c = tid + NXR * nthr; c < nch8; c += nthr)
            *reinterpret_cast<uint4v *>(xs + xs_slot(c)) = *reinterpret_cast<const uint4v *>(x + c * 8);
        __syncthreads();
    }

    float acc[R];
#pragma unroll
    for (int r = 0; r < R; r++) acc[r] = 0.f;

    // operands of the RoPE epilogue, requested when a row group starts so that their round trips overlap the stream (gemv_parts.h)
    GemvRope<bf16_t, R> rope(a, a.bias, N);
    if constexpr (EPI == EPI_QKV_ROPE) {
        rope.begin(a.st, a.max_pos);
        if (gw < ngroups) rope.prefetch(gw);
    }

    GemvBest best;                                                                  // running ArgMax of this wave's rows (lane 0)
    auto finish_group = [&](int g) {
        float sum[R];
#pragma unroll
        for (int r = 0; r < R; r++) { sum[r] = wave_sum(acc[r]) * inv_m; acc[r] = 0.f; }
        if (lane != 0) return;
        if constexpr (EPI == EPI_GATEUP) gemv_store_gateup<bf16_t, R>(reinterpret_cast<bf16_t *>(a.out), N, g, sum);
        else if constexpr (EPI == EPI_QKV_ROPE) rope.store(g, sum);
        else gemv_store_f32<R>(reinterpret_cast<float *>(a.out), a.bias, N, g, sum, a.amax != nullptr, best);
    };
    auto leave_candidate = [&]() {
        if constexpr (EPI != EPI_F32) return;
        if (a.amax) gemv_leave_candidate(a.amax, cv, ci, 0, nwv, best);              // (kernel argument: uniform)
    };

    // one chunk (one MX block) of every row against its x: sixteen converts and sixteen dots per row
    auto dot_chunk = [&](const Buf &buf, int u, const uint4v (&xp)[4]) {
#pragma unroll
        for (int r = 0; r < R; r++) {
            const float sc = __uint_as_float((((unsigned)buf.e[r] >> (8 * u)) & 0xffu) << 23);
#pragma unroll
            for (int d = 0; d < 4; d++) {
                const unsigned w = buf.w[r][u][d];
                acc[r] = dot2c_bf16(e2m1x2_to_bf16x2<0>(w, sc), xp[d][0], acc[r]);
                acc[r] = dot2c_bf16(e2m1x2_to_bf16x2<1>(w, sc), xp[d][1], acc[r]);
                acc[r] = dot2c_bf16(e2m1x2_to_bf16x2<2>(w, sc), xp[d][2], acc[r]);
                acc[r] = dot2c_bf16(e2m1x2_to_bf16x2<3>(w, sc), xp[d][3], acc[r]);
            }
        }
    };

    int cg = gw, cb = 0;                                                            // consume stream
    const bool ragged = nchunk % (64 * U) != 0;
    auto consume = [&](const Buf &buf) {
        if constexpr (EPI == EPI_QKV_ROPE) { if (cb == 0 && cg != gw) rope.prefetch(cg); }
        const int c0 = lane + 64 * U * cb;
        if (ragged && cb == nb - 1) {                                               // wave-uniform: the partial last block of K
#pragma unroll
            for (int u = 0; u < U; u++) {
                const int cc = c0 + 64 * u, cl = min(cc, nchunk - 1);
                uint4v xp[4];
#pragma unroll
                for (int d = 0; d < 4; d++) {
                    xp[d] = *reinterpret_cast<const uint4v *>(xs + d * poff + cl * 8);
                    if (cc >= nchunk) xp[d] = uint4v{0u, 0u, 0u, 0u};
                }
                dot_chunk(buf, u, xp);
            }
#pragma unroll
            for (int r = 0; r < R; r++) dot2c_settle(acc[r]);                       // (inside the branch: nothing but dots and the wait between a dot and what reads it)
        } else {
#pragma unroll
            for (int u = 0; u < U; u++) {
                const int cc = c0 + 64 * u;
                uint4v xp[4];
#pragma unroll
                for (int d = 0; d < 4; d++) xp[d] = *reinterpret_cast<const uint4v *>(xs + d * poff + cc * 8);
                dot_chunk(buf, u, xp);
            }
#pragma unroll
            for (int r = 0; r < R; r++) dot2c_settle(acc[r]);
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
    leave_candidate();
}

bool gemv_w4_supported(int64_t N, int64_t K) {
    return N > 0 && K >= 32 && K % 32 == 0 && (size_t)K * 2 <= 160 * 1024 - 256;
}
bool gemv_w4_norm_supported(int64_t N, int64_t K) { return gemv_w4_supported(N, K) && K <= 6144; }

static size_t w4_lds(int64_t K) { return ((size_t)K * 2 + 15) & ~(size_t)15; }
// the rule of the bf16 stream (gemv_geometry.h) without the fl_tune grid, over row groups of four
static GemvGeometry w4_geometry(int64_t N, int64_t K) { return gemv_geometry((N + kW4R - 1) / kW4R, w4_lds(K), device_cu_count(), 0, 0); }

bool gemv_w4_leaves_candidates(int64_t N, int64_t K) { return w4_geometry(N, K).blocks + 1 <= kMaxArgmaxCand; }

template <int U, int PRO, int EPI>
static int launch_gemv_w4_ke(Launcher &L, const GemvArgs &a, const uint8_t *escale, int blocks, int waves, size_t lds) {
    auto kern = gemv_w4_kernel<kW4R, U, PRO, EPI>;
    FL_TRY(raise_dynamic_lds(reinterpret_cast<const void *>(kern), lds));
    char tag[32];
    snprintf(tag, sizeof tag, "%dx%d%s%s,w4", a.N, a.K, PRO == PRO_NORM ? ",norm" : "", EPI == EPI_GATEUP ? ",glu" : (EPI == EPI_QKV_ROPE ? ",rope" : ""));
    Launcher LL = L; LL.tag = tag;
    return LL.launch(KC_GEMV, (double)a.N * (a.K / 2 + mx4_scale_stride(a.K)), 2.0 * a.N * a.K, kern, dim3((unsigned)blocks), dim3((unsigned)waves * 64), lds, a, escale);
}
template <int U, int PRO>
static int launch_gemv_w4_k(Launcher &L, const GemvArgs &a, const uint8_t *escale, int blocks, int waves, size_t lds) {
    if (a.epi == EPI_GATEUP) return launch_gemv_w4_ke<U, PRO, EPI_GATEUP>(L, a, escale, blocks, waves, lds);
    if (a.epi == EPI_QKV_ROPE) return launch_gemv_w4_ke<U, PRO, EPI_QKV_ROPE>(L, a, escale, blocks, waves, lds);
    return launch_gemv_w4_ke<U, PRO, EPI_F32>(L, a, escale, blocks, waves, lds);
}
template <int U>
static int launch_gemv_w4_u(Launcher &L, const GemvArgs &a, const uint8_t *escale, int blocks, int waves, size_t lds) {
    return a.pro == PRO_NORM ? launch_gemv_w4_k<U, PRO_NORM>(L, a, escale, blocks, waves, lds) : launch_gemv_w4_k<U, PRO_X>(L, a, escale, blocks, waves, lds);
}

int launch_gemv_w4(Launcher &L, const GemvArgs &a, const uint8_t *escale) {
    if (a.N <= 0 || a.K <= 0 || !a.W || !escale) FL_FAIL(FL_ERR_BAD_ARGUMENT, "launch_gemv_w4: bad shape or null weights");
    if (!gemv_w4_supported(a.N, a.K)) FL_FAIL(FL_ERR_UNSUPPORTED, "launch_gemv_w4: K=%d unsupported (a multiple of 32, at most 81792)", a.K);
    if (a.pro != PRO_X && a.pro != PRO_NORM) FL_FAIL(FL_ERR_UNSUPPORTED, "launch_gemv_w4: the prologue must be PRO_X or PRO_NORM");
    if (a.pro == PRO_NORM && !gemv_w4_norm_supported(a.N, a.K)) FL_FAIL(FL_ERR_UNSUPPORTED, "fused norm needs K <= 6144");
    if (a.epi != EPI_F32 && a.epi != EPI_GATEUP && a.epi != EPI_QKV_ROPE) FL_FAIL(FL_ERR_BAD_ARGUMENT, "launch_gemv_w4: unknown epilogue");
    if (a.epi == EPI_GATEUP && a.N % 32) FL_FAIL(FL_ERR_BAD_ARGUMENT, "gate/up matrix rows must be a multiple of 32");
    if (a.ll || a.delta_nslab != 1) FL_FAIL(FL_ERR_UNSUPPORTED, "launch_gemv_w4: no fused all-reduce, no sliced delta");
    if (a.epi == EPI_QKV_ROPE && (a.d <= 0 || a.d % 2 || a.N != (a.H + 2 * a.Hkv) * a.d)) FL_FAIL(FL_ERR_BAD_ARGUMENT, "bad qkv shape");
    const size_t lds = w4_lds(a.K);
    const GemvGeometry geo = w4_geometry(a.N, a.K);
    const int blocks = geo.blocks;
    int waves = geo.waves;
    if (a.amax && blocks + 1 > kMaxArgmaxCand) FL_FAIL(FL_ERR_BAD_ARGUMENT, "launch_gemv_w4: %d workgroups exceed the ArgMax candidate buffer", blocks);
    if (a.pro == PRO_NORM && (int64_t)waves * 64 * 3 * 8 < a.K) waves = (int)((a.K + 64 * 3 * 8 - 1) / (64 * 3 * 8));   // staging capacity
    if (mx4_u(a.K) == 2) return launch_gemv_w4_u<2>(L, a, escale, blocks, waves, lds);
    return launch_gemv_w4_u<1>(L, a, escale, blocks, waves, lds);
}

// ---- quantiser ---------------------------------------------------------------------------------------------------------------
// Work is split by block: four threads per block of 32, eight weights each (one 16-byte load of a bf16 source), the block's
// absmax over two shuffles; then the exponent, W / 2^e (exact: a power of two) rounded to the e2m1 grid in plain C++ -- the
// thresholds are the grid's midpoints, each given to the neighbour whose mantissa bit is 0 -- four bytes of nibbles per
// thread, and (img non-null) the bf16 image 2^e * q.  img may be src (bf16): a thread overwrites only the eight weights it has
// read, after the block's absmax.  U = 0: scales in the logical [N][K / 32]; U = 1, 2: the kernel's stream (mx4_scale_slot),
// the slots past K / 32 of every row set to 127.
__device__ inline unsigned e2m1_round(float v) {     // 0 <= v <= 6
    return v <= 0.25f ? 0u : v < 0.75f ? 1u : v <= 1.25f ? 2u : v < 1.75f ? 3u : v <= 2.5f ? 4u : v < 3.5f ? 5u : v <= 5.0f ? 6u : 7u;
}
__device__ inline float e2m1_value(unsigned c) {     // c < 8
    return c < 2 ? 0.5f * (float)c : ldexpf(1.0f + 0.5f * (float)(c & 1), (int)(c >> 1) - 1);
}

template <typename ST>
__global__ __launch_bounds__(256) void quantize_mx4_kernel(const ST *src, int64_t N, int64_t K, uint8_t *__restrict__ q, uint8_t *__restrict__ es, int U,
                                                           bf16_t *img) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;                       // eight weights each
    const bool live = t < N * (K >> 3);
    const int64_t row = live ? t / (K >> 3) : 0, k = live ? (t - row * (K >> 3)) * 8 : 0;
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; j++) v[j] = 0.f;
    if (live) load8(src + row * K + k, v);
    float amax = 0.f;
#pragma unroll
    for (int j = 0; j < 8; j++) amax = fmaxf(amax, fabsf(v[j]));
    amax = fmaxf(amax, __shfl_xor(amax, 1, 64));
    amax = fmaxf(amax, __shfl_xor(amax, 2, 64));
    if (!live) return;
    int e = 0;
    if (amax > 0.f) {
        int x;
        const float m = frexpf(amax, &x);            // amax = m * 2^x, m in [0.5, 1); 6 = 0.75 * 2^3
        e = m <= 0.75f ? x - 3 : x - 2;
        if (e < -120) e = -120;
    }
    const float sc = ldexpf(1.0f, e), inv = ldexpf(1.0f, -e);
    unsigned word = 0;
    float o[8];
#pragma unroll
    for (int j = 0; j < 8; j++) {
        const unsigned sign = __float_as_uint(v[j]) >> 31;
        const unsigned c = e2m1_round(fabsf(v[j]) * inv);
        word |= (c | (sign << 3)) << (4 * j);
        o[j] = __uint_as_float(__float_as_uint(e2m1_value(c) * sc) | (sign << 31));
    }
    *reinterpret_cast<unsigned *>(q + row * (K >> 1) + (k >> 1)) = word;
    if (img) store8(img + row * K + k, o);
    const int64_t nchunk = K >> 5, c = k >> 5;
    const int sub = (int)(k & 31) >> 3;
    if (U == 0) {
        if (sub == 0) es[row * nchunk + c] = (uint8_t)(e + 127);
        return;
    }
    const int64_t stride = (nchunk + 64 * U - 1) / (64 * U) * (64 * U);
    if (sub == 0) es[row * stride + mx4_scale_slot(c, U)] = (uint8_t)(e + 127);
    if (sub == 1 && c == nchunk - 1)
        for (int64_t p = nchunk; p < stride; p++) es[row * stride + mx4_scale_slot(p, U)] = 127;
}

int launch_quantize_mx4(Launcher &L, int src_dtype, const void *src, int64_t N, int64_t K, uint8_t *q, uint8_t *e, bool e_stream, void *img_bf16) {
    if (N <= 0 || K <= 0 || K % 32 || N > 0x7fffffff) FL_FAIL(FL_ERR_BAD_ARGUMENT, "quantize_mx4: bad shape (K must be a multiple of 32)");
    if (!src || !q || !e) FL_FAIL(FL_ERR_BAD_ARGUMENT, "quantize_mx4: null argument");
    Launcher LL = L; LL.tag = "quantize_mx4";
    const double bytes = (double)N * K * (src_dtype == FL_DTYPE_F32 ? 4.5 : 2.5);
    const unsigned grid = (unsigned)((N * (K >> 3) + 255) / 256);
    const int U = e_stream ? mx4_u(K) : 0;
    if (src_dtype == FL_DTYPE_BF16)
        return LL.launch(KC_CONVERT, bytes, 0.0, quantize_mx4_kernel<bf16_t>, dim3(grid), dim3(256), 0, reinterpret_cast<const bf16_t *>(src), N, K, q, e, U,
                         reinterpret_cast<bf16_t *>(img_bf16));
    if (src_dtype == FL_DTYPE_F32)
        return LL.launch(KC_CONVERT, bytes, 0.0, quantize_mx4_kernel<float>, dim3(grid), dim3(256), 0, reinterpret_cast<const float *>(src), N, K, q, e, U,
                         reinterpret_cast<bf16_t *>(img_bf16));
    FL_FAIL(FL_ERR_UNSUPPORTED, "quantize_mx4: source must be bf16 or f32");
}

// fl_op_gemv_w4: nibbles and scales in the logical layouts -> the device rows and the scale stream.  I > 0: the 2 I rows are
// gate [0, I) | up [I, 2 I) in HF order and go to the 16-interleaved layout of the decode step; I = 0: rows stay where they are.
// The caller zeroes the padding rows' nibbles and fills the whole scale stream with 127 first.
__global__ __launch_bounds__(256) void mx4_layout_kernel(const uint8_t *__restrict__ q, const uint8_t *__restrict__ e, int64_t I, int64_t K, int U,
                                                         int64_t stride, uint8_t *__restrict__ qo, uint8_t *__restrict__ eo) {
    const int64_t src = blockIdx.x;
    const int is_up = I > 0 && src >= I;
    const int64_t dst = I > 0 ? gateup_row(is_up ? src - I : src, is_up) : src;
    const int64_t kb = K >> 1, nchunk = K >> 5;
    for (int64_t k = (int64_t)threadIdx.x * 16; k < kb; k += 256 * 16)
        *reinterpret_cast<uint4v *>(qo + dst * kb + k) = *reinterpret_cast<const uint4v *>(q + src * kb + k);
    for (int64_t c = threadIdx.x; c < nchunk; c += 256) eo[dst * stride + mx4_scale_slot(c, U)] = e[src * nchunk + c];
}
int launch_mx4_layout(Launcher &L, const uint8_t *q, const uint8_t *e, int64_t N, int64_t I, int64_t K, uint8_t *qo, uint8_t *eo) {
    if (N <= 0 || K <= 0 || K % 32 || (I > 0 && N != 2 * I)) FL_FAIL(FL_ERR_BAD_ARGUMENT, "mx4_layout: bad shape");
    return L.launch(KC_CONVERT, (double)N * K * 17 / 16, 0.0, mx4_layout_kernel, dim3((unsigned)N), dim3(256), 0, q, e, I, K, mx4_u(K), mx4_scale_stride(K), qo, eo);
}

}  // namespace fl
