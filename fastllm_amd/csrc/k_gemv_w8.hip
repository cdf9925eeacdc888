// k_gemv_w8.hip -- the decode (T = 1) weight stream over FP8 weights, and the quantiser that makes them.
//
// Format (FL_WEIGHTS_E4M3_ROW): W'[n,k] = s[n] * q[n,k], q OCP e4m3fn, s[n] = 2^e one fp32 scale per output row, e the smallest
// integer with absmax(W[n,:]) / 2^e <= 448 (an all-zero row: s = 1).  The division is by a power of two, so q is defined bit
// for bit, and s * q is exactly representable in bf16: an FP8 model is the bf16 model whose weights are W'.
//
// The kernel is the sibling of k_gemv.hip's bf16 stream: same GemvArgs, and the row map, norm prologue and epilogues are the ones
// of gemv_parts.h; the stream is its own.  What differs:
//   - a lane's 16-byte load is 16 weights, so a wave instruction (1 KiB, non-temporal, straight to VGPRs) covers 1024 columns of
//     a row and a row is half as many instructions long; the wave's (row group, K block) items form one stream, a block
//     (U x R KiB) ahead in a second register buffer, every load unconditional (counted vmcnt waits), as in the bf16 PIPE form.
//     A projection with one item per wave (Mistral-7B QKV: 3072 groups of 2 rows x 4 KiB on 256 x 12 waves) has its whole
//     share requested before the prologue -- what the bf16 kernel needs its SMALL form for.
//   - conversion: v_cvt_scalef32_pk_bf16_fp8 (scale 1.0) turns two e4m3 into a packed bf16 pair, exactly; the pair goes into
//     v_dot2c_f32_bf16 against the bf16 x of LDS (common.h: dot2c_bf16 / dot2c_settle carry the dot-result hazard wait).
//     16 VALU instructions per 16 weights (8 converts + 8 dots), against 24 + the x unpack for v_cvt_pk_f32_fp8 + FMA.
//   - x in LDS is split in two halves (elements 0-7 of every 16-element chunk | elements 8-15), so that both ds_read_b128 of a
//     lane's chunk are 16-byte strided across the wave.
//   - the row scale multiplies the reduced sum in the epilogue, beside 1/rms; it is requested when the row group starts.
// K must be a multiple of 16 (a lane's load); fl_model_create_opts refuses other shapes in this mode.
#include <stdlib.h>

#include "gemv_geometry.h"
#include "gemv_parts.h"
#include "kernels.h"

namespace fl {

constexpr int kW8MaxThreads = 768;       // 12 waves: 170 VGPRs per lane
typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
typedef float f32x2_t __attribute__((ext_vector_type(2)));

// two e4m3 of `w` (bytes 0-1, or 2-3) as a packed bf16 pair
template <bool HI> __device__ inline unsigned e4m3x2_to_bf16x2(unsigned w) {
    return __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w, 1.0f, HI));
}

template <int R, int U, int PRO, int EPI>
__global__ __launch_bounds__(kW8MaxThreads) void gemv_w8_kernel(const GemvArgs a, const float *__restrict__ wscale) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    __shared__ float red[kW8MaxThreads / 64];
    __shared__ float cv[kW8MaxThreads / 64];         // ArgMax candidates of the waves (GemvArgs::amax)
    __shared__ int ci[kW8MaxThreads / 64];
    bf16_t *xs = reinterpret_cast<bf16_t *>(lds_raw);
    const uint8_t *__restrict__ W = reinterpret_cast<const uint8_t *>(a.W);
    const int N = a.N, K = a.K;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nthr = blockDim.x, nwv = nthr >> 6;
    const int nchunk = K >> 4;                       // 16-weight chunks (a lane's load); K % 16 == 0
    const int nch8 = K >> 3;                         // 8-element chunks of the activation staging
    const int hoff = K >> 1;                         // xs: [elements 0-7 of every chunk | elements 8-15 of every chunk]
    const int half = a.d >> 1;
    const int ngroups = (N + R - 1) / R;
    const int wave_u = __builtin_amdgcn_readfirstlane(wave);
    const int gw = blockIdx.x * nwv + wave_u, nw = gridDim.x * nwv;

    auto row_of = [&](int g, int r) -> int { return gemv_row_of<EPI, R>(g, r, a.d, half); };
    auto xs_slot = [&](int c8) -> int { return ((c8 & 1) ? hoff : 0) + (c8 >> 1) * 8; };

    typedef uint4v Buf[R][U];
    Buf pre;
    const int nb = (nchunk + 64 * U - 1) / (64 * U);                                // K blocks per row group (the last may be partial)
    const int n_items = gw < ngroups ? (ngroups - gw + nw - 1) / nw * nb : 0;      // this wave's items
    int lg = gw, lb = 0;                                                            // load stream: next item = (row group, block)
    // every load is unconditional: past the end of K a lane re-reads the last chunk (its x is zeroed), a row past N re-reads row N - 1
    auto load_next = [&](Buf &buf) {
        const int g = min(lg, ngroups - 1);
#pragma unroll
        for (int r = 0; r < R; r++) {
            const int row = row_of(g, r);
            const uint8_t *wr = W + (size_t)(row < N ? row : N - 1) * K;
#pragma unroll
            for (int u = 0; u < U; u++)
                buf[r][u] = __builtin_nontemporal_load(reinterpret_cast<const uint4v *>(wr + (size_t)min(lane + 64 * (U * lb + u), nchunk - 1) * 16));
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

    // operands of the epilogue, requested when a row group starts so that their round trips overlap the stream: the rows'
    // scales, and for RoPE the position's cos / sin pairs and the bias of the pair's rows (gemv_parts.h)
    float wsc[R];
    GemvRope<bf16_t, R> rope(a, a.bias, N);
    auto group_prefetch = [&](int g) {
#pragma unroll
        for (int r = 0; r < R; r++) {
            const int row = row_of(g, r);
            wsc[r] = row < N ? wscale[row] : 0.f;
        }
        if constexpr (EPI == EPI_QKV_ROPE) rope.prefetch(g);
    };
    if constexpr (EPI == EPI_QKV_ROPE) rope.begin(a.st, a.max_pos);
    if (gw < ngroups) group_prefetch(gw);

    GemvBest best;                                                                  // running ArgMax of this wave's rows (lane 0)
    auto finish_group = [&](int g) {
        float sum[R];
#pragma unroll
        for (int r = 0; r < R; r++) { sum[r] = wave_sum(acc[r]) * inv_m * wsc[r]; acc[r] = 0.f; }
        if (lane != 0) return;
        if constexpr (EPI == EPI_GATEUP) gemv_store_gateup<bf16_t, R>(reinterpret_cast<bf16_t *>(a.out), N, g, sum);
        else if constexpr (EPI == EPI_QKV_ROPE) rope.store(g, sum);
        else gemv_store_f32<R>(reinterpret_cast<float *>(a.out), a.bias, N, g, sum, a.amax != nullptr, best);
    };
    auto leave_candidate = [&]() {
        if constexpr (EPI != EPI_F32) return;
        if (a.amax) gemv_leave_candidate(a.amax, cv, ci, 0, nwv, best);              // (kernel argument: uniform)
    };

    // one chunk of every row against its x: eight converts and eight dots per row
    auto dot_chunk = [&](const Buf &buf, int u, const uint4v xa, const uint4v xb) {
#pragma unroll
        for (int r = 0; r < R; r++) {
            const uint4v w = buf[r][u];
            acc[r] = dot2c_bf16(e4m3x2_to_bf16x2<false>(w[0]), xa[0], acc[r]);
            acc[r] = dot2c_bf16(e4m3x2_to_bf16x2<true>(w[0]), xa[1], acc[r]);
            acc[r] = dot2c_bf16(e4m3x2_to_bf16x2<false>(w[1]), xa[2], acc[r]);
            acc[r] = dot2c_bf16(e4m3x2_to_bf16x2<true>(w[1]), xa[3], acc[r]);
            acc[r] = dot2c_bf16(e4m3x2_to_bf16x2<false>(w[2]), xb[0], acc[r]);
            acc[r] = dot2c_bf16(e4m3x2_to_bf16x2<true>(w[2]), xb[1], acc[r]);
            acc[r] = dot2c_bf16(e4m3x2_to_bf16x2<false>(w[3]), xb[2], acc[r]);
            acc[r] = dot2c_bf16(e4m3x2_to_bf16x2<true>(w[3]), xb[3], acc[r]);
        }
    };

    int cg = gw, cb = 0;                                                            // consume stream
    const bool ragged = nchunk % (64 * U) != 0;
    auto consume = [&](const Buf &buf) {
        if (cb == 0 && cg != gw) group_prefetch(cg);
        const int c0 = lane + 64 * U * cb;
        if (ragged && cb == nb - 1) {                                               // wave-uniform: the partial last block of K
#pragma unroll
            for (int u = 0; u < U; u++) {
                const int cc = c0 + 64 * u, cl = min(cc, nchunk - 1);
                uint4v xa = *reinterpret_cast<const uint4v *>(xs + cl * 8);
                uint4v xb = *reinterpret_cast<const uint4v *>(xs + hoff + cl * 8);
                if (cc >= nchunk) { xa = uint4v{0u, 0u, 0u, 0u}; xb = uint4v{0u, 0u, 0u, 0u}; }
                dot_chunk(buf, u, xa, xb);
            }
#pragma unroll
            for (int r = 0; r < R; r++) dot2c_settle(acc[r]);                       // (inside the branch: nothing but dots and the wait between a dot and what reads it)
        } else {
#pragma unroll
            for (int u = 0; u < U; u++) {
                const int cc = c0 + 64 * u;
                const uint4v xa = *reinterpret_cast<const uint4v *>(xs + cc * 8);
                const uint4v xb = *reinterpret_cast<const uint4v *>(xs + hoff + cc * 8);
                dot_chunk(buf, u, xa, xb);
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

bool gemv_w8_supported(int64_t N, int64_t K) {
    return N > 0 && K >= 16 && K % 16 == 0 && (size_t)K * 2 <= 160 * 1024 - 256;
}
bool gemv_w8_norm_supported(int64_t N, int64_t K) { return gemv_w8_supported(N, K) && K <= 6144; }

constexpr int kW8R = 2;
static size_t w8_lds(int64_t K) { return ((size_t)K * 2 + 15) & ~(size_t)15; }
// the rule of the bf16 stream (gemv_geometry.h) without the fl_tune grid; a row group is half the bytes, so the same rule leaves
// half the bytes per wave and the short launches (QKV, o_proj) are one item per wave
static GemvGeometry w8_geometry(int64_t N, int64_t K) { return gemv_geometry((N + kW8R - 1) / kW8R, w8_lds(K), device_cu_count(), 0, 0); }

bool gemv_w8_leaves_candidates(int64_t N, int64_t K) { return w8_geometry(N, K).blocks + 1 <= kMaxArgmaxCand; }

template <int U, int PRO, int EPI>
static int launch_gemv_w8_ke(Launcher &L, const GemvArgs &a, const float *wscale, int blocks, int waves, size_t lds) {
    auto kern = gemv_w8_kernel<kW8R, U, PRO, EPI>;
    FL_TRY(raise_dynamic_lds(reinterpret_cast<const void *>(kern), lds));
    char tag[32];
    snprintf(tag, sizeof tag, "%dx%d%s%s,w8", a.N, a.K, PRO == PRO_NORM ? ",norm" : "", EPI == EPI_GATEUP ? ",glu" : (EPI == EPI_QKV_ROPE ? ",rope" : ""));
    Launcher LL = L; LL.tag = tag;
    return LL.launch(KC_GEMV, (double)a.N * a.K + 4.0 * a.N, 2.0 * a.N * a.K, kern, dim3((unsigned)blocks), dim3((unsigned)waves * 64), lds, a, wscale);
}
template <int U, int PRO>
static int launch_gemv_w8_k(Launcher &L, const GemvArgs &a, const float *wscale, int blocks, int waves, size_t lds) {
    if (a.epi == EPI_GATEUP) return launch_gemv_w8_ke<U, PRO, EPI_GATEUP>(L, a, wscale, blocks, waves, lds);
    if (a.epi == EPI_QKV_ROPE) return launch_gemv_w8_ke<U, PRO, EPI_QKV_ROPE>(L, a, wscale, blocks, waves, lds);
    return launch_gemv_w8_ke<U, PRO, EPI_F32>(L, a, wscale, blocks, waves, lds);
}
template <int U>
static int launch_gemv_w8_u(Launcher &L, const GemvArgs &a, const float *wscale, int blocks, int waves, size_t lds) {
    return a.pro == PRO_NORM ? launch_gemv_w8_k<U, PRO_NORM>(L, a, wscale, blocks, waves, lds) : launch_gemv_w8_k<U, PRO_X>(L, a, wscale, blocks, waves, lds);
}

int launch_gemv_w8(Launcher &L, const GemvArgs &a, const float *wscale) {
    if (a.N <= 0 || a.K <= 0 || !a.W || !wscale) FL_FAIL(FL_ERR_BAD_ARGUMENT, "launch_gemv_w8: bad shape or null weights");
    if (!gemv_w8_supported(a.N, a.K)) FL_FAIL(FL_ERR_UNSUPPORTED, "launch_gemv_w8: K=%d unsupported (a multiple of 16, at most 81792)", a.K);
    if (a.pro == PRO_NORM && !gemv_w8_norm_supported(a.N, a.K)) FL_FAIL(FL_ERR_UNSUPPORTED, "fused norm needs K <= 6144");
    if (a.epi != EPI_F32 && a.epi != EPI_GATEUP && a.epi != EPI_QKV_ROPE) FL_FAIL(FL_ERR_BAD_ARGUMENT, "launch_gemv_w8: unknown epilogue");
    if (a.epi == EPI_GATEUP && a.N % 32) FL_FAIL(FL_ERR_BAD_ARGUMENT, "gate/up matrix rows must be a multiple of 32");
    if (a.ll || a.delta_nslab != 1) FL_FAIL(FL_ERR_UNSUPPORTED, "launch_gemv_w8: no fused all-reduce, no sliced delta");
    if (a.epi == EPI_QKV_ROPE && (a.d <= 0 || a.d % 2 || a.N != (a.H + 2 * a.Hkv) * a.d)) FL_FAIL(FL_ERR_BAD_ARGUMENT, "bad qkv shape");
    const size_t lds = w8_lds(a.K);
    const GemvGeometry geo = w8_geometry(a.N, a.K);
    const int blocks = geo.blocks;
    int waves = geo.waves;
    if (a.amax && blocks + 1 > kMaxArgmaxCand) FL_FAIL(FL_ERR_BAD_ARGUMENT, "launch_gemv_w8: %d workgroups exceed the ArgMax candidate buffer", blocks);
    if (a.pro == PRO_NORM && (int64_t)waves * 64 * 3 * 8 < a.K) waves = (int)((a.K + 64 * 3 * 8 - 1) / (64 * 3 * 8));   // staging capacity
    // 1-KiB wave instructions per row, and chunks per block U in {4, 2, 1}: the one that pads the row's instruction count
    // least, ties to the larger (K = 4096: 4 -> U 4, one block; 14336: 14 -> U 2; 2048: 2 -> U 2; 5632: 6 -> U 2).  U = 7 (two
    // blocks at K = 14336) needs 112 VGPRs of stream buffers and spills under the 168-register cap of a 12-wave workgroup.
    const int ni = (int)(((a.K >> 4) + 63) / 64);
    static const int kU[] = {4, 2, 1};
    int U = 1, best_pad = 1 << 30;
    for (int u : kU) {
        const int pad = (ni + u - 1) / u * u;
        if (pad < best_pad) { best_pad = pad; U = u; }
    }
    if (U == 4) return launch_gemv_w8_u<4>(L, a, wscale, blocks, waves, lds);
    if (U == 2) return launch_gemv_w8_u<2>(L, a, wscale, blocks, waves, lds);
    return launch_gemv_w8_u<1>(L, a, wscale, blocks, waves, lds);
}

// ---- quantiser ---------------------------------------------------------------------------------------------------------------
// One workgroup per row: absmax, the power-of-two scale, then four weights per thread and round: W / s (exact) through
// v_cvt_pk_fp8_f32 (RNE, OCP e4m3fn on gfx950; |W / s| <= 448, so neither saturation nor a NaN code), and -- img non-null -- the
// bf16 image s * q.  img may be src (bf16): a thread overwrites only the four weights it has read, after the row's absmax.
// The scale's exponent is kept at -126 or above (rows whose absmax is below 2^-117: s stays a normal fp32, absmax / s falls below 224).
template <typename ST>
__global__ __launch_bounds__(256) void quantize_rows_kernel(const ST *src, int64_t K, uint8_t *__restrict__ q, float *__restrict__ s,
                                                            bf16_t *img) {
    __shared__ float red[4];
    const int64_t row = blockIdx.x;
    const ST *p = src + row * K;
    const int tid = threadIdx.x;
    float amax = 0.f;
    for (int64_t k = tid; k < K; k += 256) amax = fmaxf(amax, fabsf(elem<ST>::ld(p + k)));
    amax = wave_max(amax);
    if ((tid & 63) == 0) red[tid >> 6] = amax;
    __syncthreads();
    amax = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    int e = 0;
    if (amax > 0.f) {
        int x;
        const float m = frexpf(amax, &x);            // amax = m * 2^x, m in [0.5, 1); 448 = 0.875 * 2^9
        e = m <= 0.875f ? x - 9 : x - 8;
        if (e < -126) e = -126;
    }
    const float sc = ldexpf(1.0f, e), inv = ldexpf(1.0f, -e);
    if (tid == 0) s[row] = sc;
    for (int64_t k = (int64_t)tid * 4; k < K; k += 256 * 4) {
        float v[4];
#pragma unroll
        for (int j = 0; j < 4; j++) v[j] = elem<ST>::ld(p + k + j) * inv;
        unsigned r = 0;
        r = __builtin_amdgcn_cvt_pk_fp8_f32(v[0], v[1], r, false);
        r = __builtin_amdgcn_cvt_pk_fp8_f32(v[2], v[3], r, true);
        *reinterpret_cast<unsigned *>(q + row * K + k) = r;
        if (img) {
            const f32x2_t lo = __builtin_amdgcn_cvt_pk_f32_fp8(r, false), hi = __builtin_amdgcn_cvt_pk_f32_fp8(r, true);
            bf16_t *o = img + row * K + k;
            o[0] = float_to_bf16_bits(lo[0] * sc); o[1] = float_to_bf16_bits(lo[1] * sc);
            o[2] = float_to_bf16_bits(hi[0] * sc); o[3] = float_to_bf16_bits(hi[1] * sc);
        }
    }
}

int launch_quantize_rows(Launcher &L, int src_dtype, const void *src, int64_t N, int64_t K, uint8_t *q, float *s, void *img_bf16) {
    if (N <= 0 || K <= 0 || K % 4 || N > 0x7fffffff) FL_FAIL(FL_ERR_BAD_ARGUMENT, "quantize_rows: bad shape (K must be a multiple of 4)");
    if (!src || !q || !s) FL_FAIL(FL_ERR_BAD_ARGUMENT, "quantize_rows: null argument");
    Launcher LL = L; LL.tag = "quantize_rows";
    const double bytes = (double)N * K * (src_dtype == FL_DTYPE_F32 ? 5 : 3);
    if (src_dtype == FL_DTYPE_BF16)
        return LL.launch(KC_CONVERT, bytes, 0.0, quantize_rows_kernel<bf16_t>, dim3((unsigned)N), dim3(256), 0, reinterpret_cast<const bf16_t *>(src), K, q, s,
                         reinterpret_cast<bf16_t *>(img_bf16));
    if (src_dtype == FL_DTYPE_F32)
        return LL.launch(KC_CONVERT, bytes, 0.0, quantize_rows_kernel<float>, dim3((unsigned)N), dim3(256), 0, reinterpret_cast<const float *>(src), K, q, s,
                         reinterpret_cast<bf16_t *>(img_bf16));
    FL_FAIL(FL_ERR_UNSUPPORTED, "quantize_rows: source must be bf16 or f32");
}

// fl_op_gemv_w8's gate/up case: rows in HF order (gate rows [0, I), up rows [I, 2 I)) -> the 16-interleaved layout of the
// decode step (rows [0, 2 Ip); the caller zeroes the padding)
__global__ __launch_bounds__(256) void w8_gateup_layout_kernel(const uint8_t *__restrict__ q, const float *__restrict__ s, int64_t I, int64_t K,
                                                               uint8_t *__restrict__ qo, float *__restrict__ so) {
    const int64_t src = blockIdx.x;                  // 0 .. 2 I
    const int is_up = src >= I;
    const int64_t dst = gateup_row(is_up ? src - I : src, is_up);
    for (int64_t k = (int64_t)threadIdx.x * 16; k < K; k += 256 * 16)
        *reinterpret_cast<uint4v *>(qo + dst * K + k) = *reinterpret_cast<const uint4v *>(q + src * K + k);
    if (threadIdx.x == 0) so[dst] = s[src];
}
int launch_w8_gateup_layout(Launcher &L, const uint8_t *q, const float *s, int64_t I, int64_t K, uint8_t *qo, float *so) {
    if (I <= 0 || K <= 0 || K % 16) FL_FAIL(FL_ERR_BAD_ARGUMENT, "w8_gateup_layout: bad shape");
    return L.launch(KC_CONVERT, 2.0 * I * K * 2, 0.0, w8_gateup_layout_kernel, dim3((unsigned)(2 * I)), dim3(256), 0, q, s, I, K, qo, so);
}

}  // namespace fl
