// sampler_dev.h -- the device code of token SAMPLING: the ChaCha12 word of the seeded stream, the two left-to-right fp32 sums,
// the top-p / top-k filter and sample_all.  One body for every kernel that draws a token: select_advance (k_ops.hip: one row, a
// batch's rows) and verify_sample (k_verify_sample.hip: the rows of a sampled verify step).  Device-inline functions only, for .hip
// files; each of the two files has its own callers, so each inlines sample_all as it did when the code lived in k_ops.hip.
#pragma once

#include "kernels.h"

namespace fl {

// rand_chacha ChaCha12 block `counter` (64-bit block counter, stream id 0) of the stream keyed by `key`
__device__ inline uint32_t rotl32(uint32_t x, int n) { return (x << n) | (x >> (32 - n)); }
__device__ inline uint32_t chacha12_word(const uint32_t *key, uint64_t word_index) {
    uint32_t s[16] = {0x61707865u, 0x3320646eu, 0x79622d32u, 0x6b206574u};
#pragma unroll
    for (int i = 0; i < 8; i++) s[4 + i] = key[i];
    const uint64_t counter = word_index >> 4;
    s[12] = (uint32_t)counter; s[13] = (uint32_t)(counter >> 32); s[14] = 0; s[15] = 0;
    uint32_t x[16];
#pragma unroll
    for (int i = 0; i < 16; i++) x[i] = s[i];
#define FL_QR(a, b, c, d) \
    a += b; d ^= a; d = rotl32(d, 16); c += d; b ^= c; b = rotl32(b, 12); \
    a += b; d ^= a; d = rotl32(d, 8);  c += d; b ^= c; b = rotl32(b, 7);
#pragma unroll
    for (int r = 0; r < 12; r += 2) {
        FL_QR(x[0], x[4], x[8], x[12])  FL_QR(x[1], x[5], x[9], x[13])
        FL_QR(x[2], x[6], x[10], x[14]) FL_QR(x[3], x[7], x[11], x[15])
        FL_QR(x[0], x[5], x[10], x[15]) FL_QR(x[1], x[6], x[11], x[12])
        FL_QR(x[2], x[7], x[8], x[13])  FL_QR(x[3], x[4], x[9], x[14])
    }
#undef FL_QR
    uint32_t out = 0;
#pragma unroll
    for (int i = 0; i < 16; i++) if ((int)(word_index & 15) == i) out = x[i] + s[i];
    return out;
}

// Left-to-right fp32 sum of p[0..V) by ONE lane -- the order of the reference's scalar loops -- with the
// other 1023 threads staging tiles of p through LDS ahead of it.  cumulative: p[i] is replaced by the
// running sum p[0]+..+p[i] (rand's WeightedIndex::new keeps exactly those).
constexpr int kSelTile = 4096;
__device__ inline float sequential_sum(float *__restrict__ p, int V, float *tiles /* 2 x kSelTile */, float *bcast, bool cumulative) {
    const int tid = threadIdx.x;
    const int ntiles = (V + kSelTile - 1) / kSelTile;
    float acc = 0.f;
    auto load_tile = [&](int t) {
        float *buf = tiles + (t & 1) * kSelTile;
        for (int j = tid; j < kSelTile; j += 1024) { const int i = t * kSelTile + j; buf[j] = i < V ? p[i] : 0.f; }
    };
    auto store_tile = [&](int t) {
        const float *buf = tiles + (t & 1) * kSelTile;
        for (int j = tid; j < kSelTile; j += 1024) { const int i = t * kSelTile + j; if (i < V) p[i] = buf[j]; }
    };
    load_tile(0);
    __syncthreads();
    for (int t = 0; t < ntiles; t++) {
        if (tid == 0) {
            float *buf = tiles + (t & 1) * kSelTile;
            const int n = min(kSelTile, V - t * kSelTile);
            // one dependent add chain; the LDS reads of the next 16 values are issued before the adds of
            // the current 16 so that their latency hides behind the chain
            int j = 0;
            float4v cur[4], nxt[4];
            if (n >= 16) for (int u = 0; u < 4; u++) cur[u] = *reinterpret_cast<const float4v *>(buf + 4 * u);
            for (; j + 16 <= n; j += 16) {
                const bool more = j + 32 <= n;
                if (more) for (int u = 0; u < 4; u++) nxt[u] = *reinterpret_cast<const float4v *>(buf + j + 16 + 4 * u);
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    float4v c;
                    c[0] = acc = __fadd_rn(acc, cur[u][0]); c[1] = acc = __fadd_rn(acc, cur[u][1]);
                    c[2] = acc = __fadd_rn(acc, cur[u][2]); c[3] = acc = __fadd_rn(acc, cur[u][3]);
                    if (cumulative) *reinterpret_cast<float4v *>(buf + j + 4 * u) = c;
                }
                if (more) for (int u = 0; u < 4; u++) cur[u] = nxt[u];
            }
            for (; j < n; j++) { acc = __fadd_rn(acc, buf[j]); if (cumulative) buf[j] = acc; }
        } else if (tid >= 64) {                      // the summing wave does nothing else
            // buffer (t+1)&1 held tile t-1: write its running sums back, then refill it with tile t+1;
            // a thread touches the same slots in both steps, so no barrier is needed between them
            if (cumulative && t >= 1) {
                const float *buf = tiles + ((t - 1) & 1) * kSelTile;
                for (int j = tid - 64; j < kSelTile; j += 960) { const int i = (t - 1) * kSelTile + j; if (i < V) p[i] = buf[j]; }
            }
            if (t + 1 < ntiles) {
                float *buf = tiles + ((t + 1) & 1) * kSelTile;
                for (int j = tid - 64; j < kSelTile; j += 960) { const int i = (t + 1) * kSelTile + j; buf[j] = i < V ? p[i] : 0.f; }
            }
        }
        __syncthreads();
    }
    if (cumulative) store_tile(ntiles - 1);
    if (tid == 0) bcast[0] = acc;
    __syncthreads();
    return bcast[0];
}

// The same left-to-right fp32 sum, bit for bit, without walking V dependent adds.
//
// While the running sum s stays inside one binade [2^k, 2^(k+1)) it is an integer multiple m*q of
// q = 2^(k-23), and fl(s + a) = (m + r)*q where r = round-to-nearest-even of a/q -- the tie (a/q = n + 1/2)
// goes by the parity of m + n, nothing else about m matters.  So a run of elements inside one binade
// advances m by an integer that depends only on the parity of the incoming m: every thread computes both
// candidates (inc[0], inc[1]) for its contiguous run in parallel, using a binade guessed from an
// ordinary block scan, and one lane then chains the 1024 runs with integer adds, checking each guess
// exactly (incoming exponent == k, outgoing m <= 2^24).  Runs that cross a binade, start at 0 or sit too
// close to a power of two to be guessed are "slow": their elements are parked in LDS and the lane adds
// them one by one in fp32.  A distribution crosses ~25 binades on its way to 1, so a few dozen runs
// are slow and the rest cost one chain step each.  A chain step is ~45 scalar instructions at a single wave's issue
// rate (one per ~5 cycles): 1024 of them took ~120 us, so each wave first composes its 64 runs (phase C0) and the
// chain is per 64-run group wherever a group is uniform.  Measured per sampled token (one workgroup): 0.15 ms at
// V = 32000, 0.34 ms at V = 152064; the one-lane walk: 0.45 / 2.6 ms.
constexpr int kSlowSlots = 56;          // LDS slots for slow runs (more fall back to global reads)
constexpr int kMaxRun = 152;            // elements per thread: V <= 1024 * 152 = 155648 (Qwen2: 152064)
struct OrderedSumLds {
    float s_in[1025];                   // exact running sum entering each run (s_in[1024] = total)
    int inc0[1024], inc1[1024];         // mantissa increment of a fast run for even / odd incoming mantissa
    short kexp[1024];                   // guessed biased exponent of a fast run, -1: slow
    short slot[1024];                   // LDS slot of a slow run, -1: read from global
    float wtot[16];
    int g_mode[16], g_ke[16], g_inc0[16], g_inc1[16];   // per 64-run group: 0 chain it, 1 uniform (one step), 2 empty
    uint32_t g_sb[16];                    // bits of the sum entering a uniform / empty group
    int nslots;
    float parked[kSlowSlots * kMaxRun];
};

// a slow run, one fp32 add at a time (wave-uniform: every lane computes the same chain)
__device__ inline uint32_t walk_run(uint32_t sbits, const float *__restrict__ p, int c0, int c1, int slot, const float *parked) {
    float s = __uint_as_float(sbits);
    if (slot >= 0) {
        const float *q = parked + slot * kMaxRun;                 // 16-byte aligned: kMaxRun % 4 == 0
        const int n = c1 - c0;
        int j = 0;
        for (; j + 8 <= n; j += 8) {                              // two b128 reads per 8 dependent adds
            const float4v a = *reinterpret_cast<const float4v *>(q + j), b = *reinterpret_cast<const float4v *>(q + j + 4);
            s = __fadd_rn(s, a[0]); s = __fadd_rn(s, a[1]); s = __fadd_rn(s, a[2]); s = __fadd_rn(s, a[3]);
            s = __fadd_rn(s, b[0]); s = __fadd_rn(s, b[1]); s = __fadd_rn(s, b[2]); s = __fadd_rn(s, b[3]);
        }
        for (; j < n; j++) s = __fadd_rn(s, q[j]);
    }
    else for (int i = c0; i < c1; i++) s = __fadd_rn(s, p[i]);
    return __float_as_uint(s);
}

__device__ inline float ordered_sum(const float *__restrict__ p, int V, OrderedSumLds &L) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int run = ((V + 1023) / 1024 + 3) & ~3;
    const int i0 = min(V, tid * run), i1 = min(V, i0 + run), n = i1 - i0;
    const bool vec = (V & 3) == 0;
    // phase A: estimated prefix (any order will do: it only picks the binade to try)
    float cs = 0.f;
    if (vec) for (int i = i0; i < i1; i += 4) { const float4v v = *reinterpret_cast<const float4v *>(p + i); cs += (v[0] + v[1]) + (v[2] + v[3]); }
    else for (int i = i0; i < i1; i++) cs += p[i];
    float inc = cs;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const float up = __shfl_up(inc, o, 64); if (lane >= o) inc += up; }
    if (tid == 0) L.nslots = 0;
    __syncthreads();
    if (lane == 63) L.wtot[wave] = inc;
    __syncthreads();
    float wbase = 0.f;
    for (int w = 0; w < wave; w++) wbase += L.wtot[w];
    const float est_out = wbase + inc, est_in = est_out - cs;
    // phase B: classify the run and, if it looks like it stays in one binade, take both increments
    const uint32_t eb = __float_as_uint(est_in) >> 23;              // biased exponent (est_in >= 0)
    const float lo = __uint_as_float(eb << 23), hi = __uint_as_float((eb + 1) << 23);
    const bool fast = n > 0 && eb > 24 && eb < 250 && est_in >= lo * 1.001f && est_out <= hi * 0.999f;
    short myslot = -1;
    if (fast) {
        const float inv_q = __uint_as_float((uint32_t)(127 + 150 - (int)eb) << 23);      // 2^(23 - k), k = eb - 127
        int a0 = 0, a1 = 1;
        auto step = [&](float a) {
            const float t = a * inv_q;                              // exact (power of two), < 2^24 in a one-binade run
            const float fl = floorf(t);
            const float fr = t - fl;                                // exact
            const int nn = (int)fl + (fr > 0.5f ? 1 : 0);
            const int tie = fr == 0.5f ? 1 : 0;
            a0 += nn + (tie & (a0 + (int)fl));
            a1 += nn + (tie & (a1 + (int)fl));
        };
        if (vec) for (int i = i0; i < i1; i += 4) { const float4v v = *reinterpret_cast<const float4v *>(p + i); step(v[0]); step(v[1]); step(v[2]); step(v[3]); }
        else for (int i = i0; i < i1; i++) step(p[i]);
        L.inc0[tid] = a0; L.inc1[tid] = a1 - 1;
        L.kexp[tid] = (short)eb;
    } else {
        L.kexp[tid] = -1;
        if (n > 0 && n <= kMaxRun) {
            const int sl = atomicAdd(&L.nslots, 1);
            if (sl < kSlowSlots) { myslot = (short)sl; for (int i = i0; i < i1; i++) L.parked[sl * kMaxRun + (i - i0)] = p[i]; }
        }
    }
    L.slot[tid] = myslot;
    __syncthreads();
    // phase C0 (all 16 waves): a wave composes its 64 runs.  The fast step m -> m + inc[m & 1] acts on the mantissa
    // parity only through inc, so two consecutive steps compose to another such pair,
    //     (L then R)[p] = L[p] + R[(p + L[p]) & 1],
    // which is associative: a wave-level scan gives every run its increment from the start of the group for either
    // entering parity, and the group's total.  A group is "uniform" when all its runs are fast in the same binade.
    const int c_me = tid, ke_me = L.kexp[c_me];
    const bool empty_me = n == 0;
    int t0 = empty_me ? 0 : L.inc0[c_me], t1 = empty_me ? 0 : L.inc1[c_me];        // inclusive transducer prefix (so far: own)
    {
        const unsigned long long fastm = __ballot(!empty_me && ke_me >= 0), usedm = __ballot(!empty_me);
        const int first = usedm ? __builtin_ctzll(usedm) : 0;
        const int ke_ref = __shfl(ke_me, first, 64);
        const bool uniform = usedm != 0 && fastm == usedm && __ballot(!empty_me && ke_me != ke_ref) == 0;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int l0 = __shfl_up(t0, o, 64), l1 = __shfl_up(t1, o, 64);
            if (lane >= o) {
                const int n0v = l0 + ((l0 & 1) ? t1 : t0), n1v = l1 + (((1 + l1) & 1) ? t1 : t0);
                t0 = n0v; t1 = n1v;
            }
        }
        if (lane == 63) { L.g_mode[wave] = usedm == 0 ? 2 : (uniform ? 1 : 0); L.g_ke[wave] = ke_ref; L.g_inc0[wave] = t0; L.g_inc1[wave] = t1; }
    }
    __syncthreads();
    // phase C1: wave 0 chains the 16 groups.  A uniform group is one integer step (checked exactly: entering
    // exponent == its binade, leaving mantissa <= 2^24); any other group is chained run by run -- per-run data in vector
    // registers (lane j = run 64g + j) read back with v_readlane, slow runs walked in fp32.
    if (wave == 0) {
        uint32_t sb = 0;                                             // bits of the running sum (>= 0)
        for (int g = 0; g < 16; g++) {
            const int mode = L.g_mode[g];
            if (mode == 2) { if (lane == 0) L.g_sb[g] = sb; continue; }
            if (mode == 1) {
                const int ke = L.g_ke[g];
                const uint32_t m = (sb & 0x7fffffu) | 0x800000u;
                const uint32_t m2 = m + (uint32_t)((m & 1) ? L.g_inc1[g] : L.g_inc0[g]);
                if ((int)(sb >> 23) == ke && m2 <= 0x1000000u) {
                    if (lane == 0) L.g_sb[g] = sb;
                    sb = ((uint32_t)ke << 23) + (m2 - 0x800000u);
                    continue;
                }
                if (lane == 0) L.g_mode[g] = 0;                      // the guess did not hold: chain it
            }
            const int c = g * 64 + lane;
            const int ke_v = L.kexp[c], a0_v = L.inc0[c], a1_v = L.inc1[c], sl_v = L.slot[c];
            uint32_t sin_v = 0;
#pragma unroll 1
            for (int j = 0; j < 64; j++) {
                if (lane == j) sin_v = sb;
                const int c0 = min(V, (g * 64 + j) * run), c1 = min(V, c0 + run);
                const int ke = __builtin_amdgcn_readlane(ke_v, j);
                const int a0 = __builtin_amdgcn_readlane(a0_v, j), a1 = __builtin_amdgcn_readlane(a1_v, j);
                // branch-free fast step: the new bits are (ke << 23) + (m2 - 2^23), also right when m2 == 2^24
                const uint32_t m = (sb & 0x7fffffu) | 0x800000u;
                const uint32_t m2 = m + (uint32_t)(a0 + (int)(m & 1) * (a1 - a0));
                const bool ok = (ke >= 0) & ((int)(sb >> 23) == ke) & (m2 <= 0x1000000u);
                const uint32_t fast_sb = ((uint32_t)ke << 23) + (m2 - 0x800000u);
                if (!ok && c0 < c1) sb = __builtin_amdgcn_readfirstlane(walk_run(sb, p, c0, c1, __builtin_amdgcn_readlane(sl_v, j), L.parked));
                else sb = (ok & (c0 < c1)) ? fast_sb : sb;
            }
            L.s_in[c] = __uint_as_float(sin_v);
        }
        if (lane == 0) L.s_in[1024] = __uint_as_float(sb);
    }
    __syncthreads();
    // phase C2 (all waves): runs of a uniform group get their entering sum from the group's and their scan prefix
    {
        const int mode = L.g_mode[wave];
        if (mode != 0) {
            const uint32_t gsb = L.g_sb[wave];
            uint32_t mine = gsb;
            if (mode == 1) {
                const int e0 = __shfl_up(t0, 1, 64), e1 = __shfl_up(t1, 1, 64);        // exclusive prefix = inclusive of lane - 1
                const uint32_t m = (gsb & 0x7fffffu) | 0x800000u;
                const int excl = lane == 0 ? 0 : ((m & 1) ? e1 : e0);
                mine = ((uint32_t)L.g_ke[wave] << 23) + (m + (uint32_t)excl - 0x800000u);
            }
            L.s_in[tid] = __uint_as_float(mine);
        }
    }
    __syncthreads();
    return L.s_in[1024];
}

// Sampling::TopP / TopK / TopKThenTopP (candle-transformers 0.8 generation::LogitsProcessor) [UPSTREAM-RECALLED]: between
// the normalisation and the cumulative weights of sample_all, everything outside the kept prefix of the sorted order
// (prs descending, the lower index first among equals: candle's stable sort) is zeroed.  The prefix ends at the first
// element whose SEQUENTIAL fp32 running sum (from 0, in sorted order) is not < top_p, or at rank top_k, whichever comes
// first -- the sum is walked by one lane over exactly sorted keys; the parallel passes only pick what to sort.
//
// A key is (bits(prs) << 1) : ~index, a total order over distinct keys whose descending order is the sorted order.
// The vocabulary is taken in descending BANDS of at most kBandKeys keys: a band is [lo, hi) in key space, hi the lower
// end of the band before it.  lo comes from a 256-bin histogram of the keys below hi over the top byte (the exponent):
// as many whole bins from the top as fit.  Only when the top non-empty bin alone is too large (a flat region, ties)
// is it split by the next byte, and so on down to the index bytes, where a bin holds one key.  The band is gathered
// into LDS, sorted (bitonic), and walked with the running sum carried in from the band before: no cap on the nucleus.
// LDS: the block OrderedSumLds occupies, free between the two sums.
constexpr int kBandKeys = 4096;
struct TopFilterLds {
    unsigned long long keys[kBandKeys];
    unsigned hist[16][256];             // per wave, then [0][] = the workgroup's
    unsigned long long lo, hi, prefix, cut;
    unsigned n, walked, found, refine;
    float acc;
};

__device__ inline unsigned long long top_key(float v, int i) {
    return ((unsigned long long)(__float_as_uint(v) << 1) << 32) | (unsigned)~(unsigned)i;
}

__device__ inline void top_filter(float *__restrict__ p, int V, SampleState *__restrict__ ss, TopFilterLds *__restrict__ F) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float top_p = ss->top_p;                     // +inf: no top-p
    const unsigned top_k = ss->top_k;                  // >= V: no top-k
    if (tid == 0) { F->hi = ~0ull; F->walked = 0; F->found = 0; F->acc = 0.f; F->cut = 0; }
    __syncthreads();
    for (int band = 0; band < V; band++) {             // (every band holds at least one key)
        const unsigned long long hi = F->hi;
        // ---- lo: whole histogram bins from the top while they fit; a level deeper only if the top bin alone does not
        unsigned long long prefix = 0;
        bool have = false;
        for (int level = 0; level < 8 && !have; level++) {
            const int shift = 56 - 8 * level;
            for (int j = tid; j < 16 * 256; j += 1024) (&F->hist[0][0])[j] = 0;
            __syncthreads();
            for (int i0 = 0; i0 < V; i0 += 1024) {
                const int i = i0 + tid;
                unsigned long long key = 0;
                bool act = false;
                if (i < V) { key = top_key(p[i], i); act = key < hi && (level == 0 || (key >> (shift + 8)) == prefix); }
                const int d = (int)((key >> shift) & 255);
                const unsigned long long am = __ballot(act);
                if (am) {                              // a wave whose keys share the bin (flat regions) adds once
                    const int first = __builtin_ctzll(am);
                    const int d0 = __shfl(d, first, 64);
                    if (__ballot(act && d != d0) == 0) { if (lane == first) atomicAdd(&F->hist[wave][d0], (unsigned)__builtin_popcountll(am)); }
                    else if (act) atomicAdd(&F->hist[wave][d], 1u);
                }
            }
            __syncthreads();
            if (tid < 256) { unsigned s = 0; for (int w = 0; w < 16; w++) s += F->hist[w][tid]; F->hist[0][tid] = s; }
            __syncthreads();
            if (tid == 0) {
                int d = 255;
                while (d > 0 && F->hist[0][d] == 0) d--;
                unsigned cum = F->hist[0][d];
                if (cum > (unsigned)kBandKeys) { F->refine = 1; F->prefix = (prefix << 8) | (unsigned)d; }
                else {
                    while (d > 0 && cum + F->hist[0][d - 1] <= (unsigned)kBandKeys) { d--; cum += F->hist[0][d]; }
                    F->refine = 0; F->lo = ((prefix << 8) | (unsigned)d) << shift; F->n = 0;
                }
            }
            __syncthreads();
            if (F->refine) prefix = F->prefix; else have = true;
        }
        if (!have) break;                              // (cannot happen: at the last level a bin holds one key)
        const unsigned long long lo = F->lo;
        // ---- gather [lo, hi) into LDS (any order), pad to a power of two with key 0 (below every real key)
        for (int i0 = 0; i0 < V; i0 += 1024) {
            const int i = i0 + tid;
            unsigned long long key = 0;
            if (i < V) key = top_key(p[i], i);
            const bool act = i < V && key >= lo && key < hi;
            const unsigned long long am = __ballot(act);
            if (am) {
                unsigned base = 0;
                const int first = __builtin_ctzll(am);
                if (lane == first) base = atomicAdd(&F->n, (unsigned)__builtin_popcountll(am));
                base = __shfl(base, first, 64);
                const unsigned at = base + (unsigned)__builtin_popcountll(am & ((1ull << lane) - 1));
                if (act && at < (unsigned)kBandKeys) F->keys[at] = key;
            }
        }
        __syncthreads();
        const int n = (int)min(F->n, (unsigned)kBandKeys);
        if (n == 0) break;                             // (cannot happen while keys remain below hi)
        int np = 1;
        while (np < n) np <<= 1;
        for (int j = n + tid; j < np; j += 1024) F->keys[j] = 0;
        __syncthreads();
        // ---- bitonic sort, descending
        for (int k = 2; k <= np; k <<= 1) {
            for (int j = k >> 1; j > 0; j >>= 1) {
                for (int t = tid; t < np / 2; t += 1024) {
                    const int a = ((t & ~(j - 1)) << 1) | (t & (j - 1)), b = a | j;
                    const unsigned long long ka = F->keys[a], kb = F->keys[b];
                    if ((ka < kb) == ((a & k) == 0)) { F->keys[a] = kb; F->keys[b] = ka; }
                }
                __syncthreads();
            }
        }
        // ---- one lane walks the band: the sequential fp32 sum of the sorted order, carried from the band before
        if (tid == 0) {
            float acc = F->acc;
            unsigned r = F->walked;
            const unsigned long long *ks = F->keys;
            auto val = [](unsigned long long key) { return __uint_as_float((unsigned)(key >> 32) >> 1); };
            int j = 0, hit = -1;
            // eight adds per look at the stop conditions (the sums only grow, so the last of the eight decides); the next
            // eight keys are read before the adds of the current eight
            unsigned long long cur[8], nxt[8];
            if (n >= 8) for (int u = 0; u < 8; u++) cur[u] = ks[u];
            for (; j + 8 <= n; j += 8) {
                const bool more = j + 16 <= n;
                if (more) for (int u = 0; u < 8; u++) nxt[u] = ks[j + 8 + u];
                float c[8];
                float a = acc;
#pragma unroll
                for (int u = 0; u < 8; u++) c[u] = a = __fadd_rn(a, val(cur[u]));
                if (!(a < top_p) || r + 8 >= top_k) {
#pragma unroll
                    for (int u = 0; u < 8; u++) if (hit < 0 && (!(c[u] < top_p) || r + u + 1 >= top_k)) hit = j + u;
                    break;
                }
                acc = a; r += 8;
                if (more) for (int u = 0; u < 8; u++) cur[u] = nxt[u];
            }
            if (hit < 0)
                for (; j < n; j++) { acc = __fadd_rn(acc, val(ks[j])); r++; if (!(acc < top_p) || r >= top_k) { hit = j; break; } }
            if (hit >= 0) { F->found = 1; F->cut = ks[hit]; F->walked = F->walked + (unsigned)hit + 1; }
            else { F->acc = acc; F->walked = r; F->hi = lo; }
        }
        __syncthreads();
        if (F->found || F->walked >= (unsigned)V) break;
    }
    // ---- mask: everything after the last kept key of the sorted order is zeroed
    const bool found = F->found != 0;
    const unsigned long long cut = F->cut;
    if (found) for (int i = tid; i < V; i += 1024) { const float v = p[i]; if (top_key(v, i) < cut) p[i] = 0.f; }
    if (tid == 0) ss->kept = found ? F->walked : (unsigned)V;
    __syncthreads();
}

// Sampling::All { temperature } (candle-transformers LogitsProcessor over rand 0.8's WeightedIndex<f32>):
//   prs = softmax(logits * (f32)(1/temperature));  total = sum(prs);  chosen = uniform[0,1) * total with
//   uniform = f32::from_bits((next_u32() >> 9) | 0x3f800000) - 1;  token = #{ j < V-1 : prs[0]+..+prs[j] <= chosen }.
// Both sums of the reference (softmax denominator: candle's scalar vec_sum in a default build; cumulative
// weights: WeightedIndex::new) run left to right in fp32, and at V ~ 1e5 that order is visible in the
// result (small terms are absorbed: the sequential total is off by ~4e-5, several tokens wide in a flat
// region), so the two sums are done in that order by one lane; max / exp / divide / count are parallel.
// exp is evaluated in fp64 and rounded, which reproduces a correctly rounded expf (glibc's, which Rust's
// f32::exp calls) except in ~1e-9 of the cases.
__device__ inline int sample_all(const float *__restrict__ logits, int V, SampleState *__restrict__ ss, float *__restrict__ p,
                                 float *red, unsigned char *lds, float *bcast, int *count) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float mul = ss->inv_temp;
    // on == 1: ordered_sum (parallel, bit-identical to the walk); on == 2 or a vocabulary beyond its run
    // size: sequential_sum (the plain walk, kept as the cross-check)
    const bool walk = ss->on == 2 || V > 1024 * kMaxRun;
    OrderedSumLds &L = *reinterpret_cast<OrderedSumLds *>(lds);
    float *tiles = reinterpret_cast<float *>(lds);
    float mx = -INFINITY;
    for (int i = tid; i < V; i += 1024) mx = fmaxf(mx, __fmul_rn(logits[i], mul));
    mx = wave_max(mx);
    if (lane == 0) red[wave] = mx;
    __syncthreads();
    mx = red[0];
    for (int w = 1; w < 16; w++) mx = fmaxf(mx, red[w]);
    for (int i = tid; i < V; i += 1024) p[i] = (float)exp((double)__fsub_rn(__fmul_rn(logits[i], mul), mx));
    __syncthreads();
    const float S = walk ? sequential_sum(p, V, tiles, bcast, false) : ordered_sum(p, V, L);
    for (int i = tid; i < V; i += 1024) p[i] = __fdiv_rn(p[i], S);
    if (tid == 0) *count = 0;
    __syncthreads();
    if (ss->filter) top_filter(p, V, ss, reinterpret_cast<TopFilterLds *>(lds));       // Sampling::TopP / TopK / TopKThenTopP
    // walk: p[] is replaced by the cumulative weights; ordered: L.s_in[] holds the sum entering every run
    const float total = walk ? sequential_sum(p, V, tiles, bcast, true) : ordered_sum(p, V, L);
    if (tid == 0) {
        // UniformFloat::new(0, total): scale = total, lowered by ulps while scale * (1 - 2^-23) >= total
        float scale = total;
        while (__fmul_rn(scale, 1.0f - 1.1920929e-07f) >= total) scale = __uint_as_float(__float_as_uint(scale) - 1);
        const uint64_t w = ((uint64_t)ss->draw_hi << 32) | ss->draw_lo;
        const uint32_t u = chacha12_word(ss->key, w);
        ss->draw_lo = (uint32_t)(w + 1); ss->draw_hi = (uint32_t)((w + 1) >> 32);
        bcast[1] = __fmul_rn(__fsub_rn(__uint_as_float((u >> 9) | 0x3f800000u), 1.0f), scale);
    }
    __syncthreads();
    const float chosen = bcast[1];
    // partition_point: how many cumulative weights are <= chosen (chosen < total, so the last one never is)
    int n = 0;
    if (walk) {
        for (int i = tid; i < V - 1; i += 1024) n += p[i] <= chosen ? 1 : 0;
    } else {
        const int run = ((V + 1023) / 1024 + 3) & ~3;
        const int i0 = min(V, tid * run), i1 = min(V, i0 + run);
        if (i0 < i1) {
            if (L.s_in[tid + 1] <= chosen) n = i1 - i0;            // the whole run is below (sums only grow)
            else if (L.s_in[tid] <= chosen) {                       // the boundary run: walk it from its exact start
                float cum = L.s_in[tid];
                for (int i = i0; i < i1; i++) { cum = __fadd_rn(cum, p[i]); if (cum <= chosen) n++; else break; }
            }
        }
    }
    for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o, 64);
    if (lane == 0 && n) atomicAdd(count, n);
    __syncthreads();
    return min(*count, V - 1);
}

constexpr size_t kSelLds = sizeof(OrderedSumLds) > 2 * kSelTile * 4 ? sizeof(OrderedSumLds) : 2 * kSelTile * 4;
static_assert(sizeof(TopFilterLds) <= kSelLds, "the top-p / top-k filter lives in the LDS block of the ordered sums");

}  // namespace fl
