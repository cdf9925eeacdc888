// attn_prefill16.h -- the ONE device body of the 16-row MFMA prefill attention: attn_prefill_mfma_kernel (k_attn_mfma.hip, one
// prompt, its cache passed in) and attn_prefill_packed_mfma_kernel (k_prefill_packed.hip, the workgroup's sequence looked up in the
// pack's table) resolve their sequence into a Prefill16Seq and call it.  What differs between them is where that view comes from and,
// in the key-split form, from which tile the wave pair's alternation is counted (OWN_ORIGIN).
#pragma once
#include "attn_mfma.h"

namespace fl {

// One sequence as a workgroup sees it.  q / out: the sequence's own rows [T][H*D]; kb / vb: the K rows [seq_alloc][D] and V^T rows
// [D][seq_alloc] of this workgroup's kv head; T new tokens behind len cached keys, of which [0, c0) came before the API call;
// tb0: the workgroup's first token.  Everything is wave-uniform.
struct Prefill16Seq { const bf16_t *q, *kb, *vb; bf16_t *out; int T, len, c0, seq_alloc, tb0; };

// one output row: (val(db) for the row's D / 16 column blocks) / l -> bf16, unless the token lies past the sequence's end
template <int D, typename F>
__device__ __forceinline__ void prefill16_store_row(bf16_t *out, int tt, int T, int H, int hq, int i, float l, F val) {
    if (tt >= T) return;
    const float inv = 1.0f / l;
    bf16_t *o = out + ((size_t)tt * H + hq) * D;
#pragma unroll
    for (int db = 0; db < D / 16; db++) o[db * 16 + i] = float_to_bf16_bits(val(db) * inv);
}

// Workgroup = G * TT (* KS) waves: wave w serves query head w % G of kv head hk for the 16 tokens of sub-tile (w / G) % TT.  All waves
// walk the same key tiles of 32 keys, staged ONCE per workgroup in LDS by LDS-DMA (K tile + V^T tile), so every K/V byte fetched from
// L2 feeds G * TT x 16 query rows.  Columns past the sequence's end carry q = 0 and are not stored.  A wave skips the tiles wholly
// outside its own visible range (wstart / wend); staging is never skipped.
// Mask (App. A.5): the keys cached before the API call [0, c0) are an unmasked prefix; the causal + sliding-window mask runs over the
// call's own tokens (c0 <= len: the library may have cut the call into chunks; a packed call never is, c0 == len).
// KS == 1: a ring of nst tiles, nst - 1 of them in flight.
// KS == 2 (short prompts): two waves per (head, sub-tile) take alternate key tiles and merge through LDS at the end -- a key step is a
// chain of dependent latencies, and this puts two such chains on every SIMD.  Which of the pair takes a tile is counted from the
// workgroup's first staged tile (kstart; OWN_ORIGIN false, the single prompt) or from the WAVE's own first useful tile (wstart;
// OWN_ORIGIN true, the pack: the split then depends on the wave's own 16 tokens only, not on TT or the rest of the pack).  At TT = 1
// wstart == kstart and the two agree.
// FULL (the packed kernel's full-mask instantiations only, fl_batch_embed's FL_MASK_FULL): every token of the sequence sees all of
// its keys [0, len + T) and the window is ignored -- hi_q, wend and kend become len + T, lo stays c0, wstart = kstart = 0.  The keys
// past len + T inside the last 32-key tile stay masked by hi_q.  Every wave walks all tiles, so the pair's alternation starts at
// tile 0 for every wave.
template <int D, int KS, bool OWN_ORIGIN, bool FULL = false>
__device__ __forceinline__ void prefill16_body(const Prefill16Seq v, int hk, int H, int Hkv, float scale, int window, int TT, int nst,
                                               unsigned char *lds) {      // lds: nst x KS x (K tile | V^T tile)
    constexpr int TILE = 2 * 32 * D * 2;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), nwv = blockDim.x >> 6;
    const int i = lane & 15, g4 = lane >> 4;
    const int G = H / Hkv;
    const int wq = wave % (G * TT), half = wave / (G * TT);      // (half: KS == 2 only)
    const int hq = hk * G + wq % G;
    const int T = v.T, len = v.len, c0 = v.c0, seq_alloc = v.seq_alloc, tb0 = v.tb0;
    const int t0 = tb0 + (wq / G) * 16;                          // first token of this wave
    const int t = t0 + i;                                        // this lane's column
    const bool col_ok = t < T;

    bf16x8 qf[D / 32];
#pragma unroll
    for (int dk = 0; dk < D / 32; dk++) {
        if (col_ok) qf[dk] = ld_bf16x8(v.q + ((size_t)t * H + hq) * D + dk * 32 + g4 * 8);
        else {
#pragma unroll
            for (int j = 0; j < 8; j++) qf[dk][j] = (__bf16)0.f;
        }
    }
    int lo = c0;
    if (!FULL && window >= 0 && len + t - window > c0) lo = len + t - window;
    const int lo_q = col_ok ? lo : 0, hi_q = col_ok ? (FULL ? len + T : len + t + 1) : 0;
    const int pre_hi = col_ok ? c0 : 0;
    // this wave's useful key range (uniform per wave): tiles outside are skipped, staging is not
    int wstart = 0;
    if (!FULL && c0 == 0 && window >= 0 && len + t0 - window > 0) wstart = ((len + t0 - window) / 32) * 32;
    const int wend = t0 < T ? len + (FULL ? T : min(T, t0 + 16)) : 0;

    MfmaAttnState<D> s; s.init();
    const bf16_t *kb = v.kb, *vb = v.vb;
    int kstart = 0;
    if (!FULL && c0 == 0 && window >= 0 && len + tb0 - window > 0) kstart = ((len + tb0 - window) / 32) * 32;
    const int kend = len + (FULL ? T : min(T, tb0 + 16 * TT));   // <= the cache's capacity <= seq_alloc (a multiple of 32)
    const int nsteps = (kend - kstart + 31) / 32;
    constexpr int NI = D / 16 + D / 16;
    const int per = (NI + nwv - 1) / nwv;
    bf16_t *out = v.out;
    if constexpr (KS == 2) {
        // super-steps of two tiles (buffers [stage][tile]); one barrier per super-step, two LDS stages
        const int nsuper = (nsteps + 1) / 2;
        const int mine = OWN_ORIGIN ? half ^ (((max(wstart, kstart) - kstart) >> 5) & 1) : half;   // this wave's tile of every super-step
        auto stage2 = [&](int ss, int stg) {
            const int k0 = kstart + 64 * ss;
            stage_kv<D>(kb, vb, seq_alloc, k0, lds + (stg * 2) * TILE, wave, nwv, lane, per);
            if (k0 + 32 < kend) stage_kv<D>(kb, vb, seq_alloc, k0 + 32, lds + (stg * 2 + 1) * TILE, wave, nwv, lane, per);
        };
        stage2(0, 0);
        for (int ss = 0; ss < nsuper; ss++) {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            if (ss + 1 < nsuper) stage2(ss + 1, (ss + 1) & 1);
            const int kbase = kstart + 64 * ss + 32 * mine;
            if (kbase < kend && kbase + 32 > wstart && kbase < wend) {               // wave-uniform
                const unsigned char *cur = lds + ((ss & 1) * 2 + mine) * TILE;
                const LdsKV<D> kv{cur, cur + 32 * D * 2, i, g4};
                attn_tile<D>(s, qf, kv, kbase, pre_hi, lo_q, hi_q, scale, lane);
            }
        }
        // merge the two key halves through LDS (the tiles are dead after the barrier)
        __syncthreads();
        float *slab = reinterpret_cast<float *>(lds) + (size_t)wq * (16 * D + 32);
        const float lt1 = mfma_l_total(s.l);
        if (half == 1) {
#pragma unroll
            for (int r = 0; r < 4; r++)
#pragma unroll
                for (int db = 0; db < D / 16; db++) slab[(4 * g4 + r) * D + db * 16 + i] = s.O[db][r];
            if (g4 == 0) { slab[16 * D + i] = s.m; slab[16 * D + 16 + i] = lt1; }
        }
        __syncthreads();
        if (half == 1) return;
        const float m1 = slab[16 * D + i], l1 = slab[16 * D + 16 + i];
        const float mm = fmaxf(s.m, m1);
        const float w0 = s.m == -INFINITY ? 0.f : __expf(s.m - mm), w1 = m1 == -INFINITY ? 0.f : __expf(m1 - mm);
        const float ltot = lt1 * w0 + l1 * w1;
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int qq = 4 * g4 + r;
            const float lr = __shfl(ltot, qq, 64), a0 = __shfl(w0, qq, 64), a1 = __shfl(w1, qq, 64);
            // (roundings spelled out: left to the compiler, ONE element of the single-prompt kernel once came out as two products and
            // an add where all the others, and the packed kernel's, were a product and an FMA -- profiles/attn_prefill16/README.md)
            prefill16_store_row<D>(out, t0 + qq, T, H, hq, i, lr,
                                   [&](int db) { return __fmaf_rn(s.O[db][r], a0, __fmul_rn(slab[qq * D + db * 16 + i], a1)); });
        }
    } else {
        for (int a = 0; a < nst - 1 && a < nsteps; a++) stage_kv<D>(kb, vb, seq_alloc, kstart + 32 * a, lds + a * TILE, wave, nwv, lane, per);
        for (int sidx = 0; sidx < nsteps; sidx++) {
            wait_vmcnt(per * min(nst - 2, nsteps - 1 - sidx));       // tile sidx has landed; the younger ones may still fly
            __builtin_amdgcn_s_barrier();
            const int kbase = kstart + 32 * sidx;
            if (sidx + nst - 1 < nsteps)
                stage_kv<D>(kb, vb, seq_alloc, kbase + 32 * (nst - 1), lds + ((sidx + nst - 1) % nst) * TILE, wave, nwv, lane, per);
            if (kbase + 32 > wstart && kbase < wend) {               // wave-uniform
                const unsigned char *cur = lds + (sidx % nst) * TILE;
                const LdsKV<D> kv{cur, cur + 32 * D * 2, i, g4};
                attn_tile<D>(s, qf, kv, kbase, pre_hi, lo_q, hi_q, scale, lane);
            }
        }
        const float lt = mfma_l_total(s.l);
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int qq = 4 * g4 + r;
            prefill16_store_row<D>(out, t0 + qq, T, H, hq, i, __shfl(lt, qq, 64), [&](int db) { return s.O[db][r]; });
        }
    }
}

}  // namespace fl
