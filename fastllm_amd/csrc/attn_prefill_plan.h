// attn_prefill_plan.h -- which MFMA prefill attention kernel a prompt (or a pack of prompts) runs, and with what launch: plain C++,
// no HIP, so that tests/test_attn_prefill_plan.py compiles it with the host compiler alone.  k_attn_mfma.hip
// (launch_attn_prefill_mfma) and k_prefill_packed.hip map a plan to a template instantiation; nothing else decides.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>

namespace fl {

// the switches of the rule (fl_tune "attn_pf32_min_t", "attn_pf32_ks2", "attn_pf32_paired", "attn_pf_waves", "attn_pf_stages",
// "attn_pf_ksplit"); the .hip side fills it from tune()
struct AttnPrefillTune { int pf32_min_t, pf32_ks2, pf32_paired, pf_waves, pf_stages, pf_ksplit; };

// The thresholds below were measured on the 256 CUs of one MI355X and count workgroups against THAT chip, whatever device runs
// the launch (the device's own CU count sizes the snake grid only).
constexpr int kPfChipCus = 256;
constexpr int kPfTwoRounds = 2 * kPfChipCus;     // (block, kv head) items from which a persistent, balanced grid pays
// Paired (balanced) 32-row grids win as soon as they cover ~3/4 of the chip -- Mistral-7B per layer: T = 3072 134 us paired (192
// workgroups) vs 197 unpaired, T = 4096 177 vs 305, T = 8192 681 vs 693; T = 2048 (128 paired workgroups) 98 vs 85.
constexpr int kPf32PairedMinWgs = 180;
// 32-row waves (attn_prefill32_kernel) once the prompt is long enough to fill the chip with their workgroups
// (with wave pairs from 640 tokens for G = 1, 2, 4: Mistral-7B T = 768 31.9 -> 24.8 us per layer, T = 512 a tie, below slower;
// from 256 tokens for the groups dealt as subgroups of four heads: Qwen2-7B T = 512 23.2 -> 18.3, TinyLlama 16.5 -> 13.2, T = 256 a tie)
// (since round 4, with four waves per (head, block) up to 576 tokens: from 352 tokens for G = 1, 2, 4 as well)
constexpr int kPf32MinT124 = 352, kPf32MinTWide = 256, kPf32MinTOther = 1024;
// (577-639 tokens, G = 1, 2, 4: the four-wave form ends at 576 tokens, the wave pairs pay from 640: the 16-row kernel in between)
constexpr int kPf32FourWaveMaxT = 576, kPf32PairMinT = 640;
constexpr size_t kPfDefaultLds = 64 * 1024;      // the LDS a launch gets without asking for more
constexpr size_t kPfTileBytes32 = 2 * 32 * 2;    // K tile + V^T tile of 32 keys, bf16: times d

// ------------------------------------------------------------------------------- the 16-row kernel's launch rule
struct Prefill16Launch { int nst; size_t lds; int block; };

inline size_t prefill16_slab_bytes(int G, int64_t d, int tt) { return (size_t)G * tt * (16 * d + 32) * 4; }

// key split (two waves per head and token sub-tile): short prompts
// (four waves per query tile measured slower than two: Mistral T = 512 23 vs 18 us per layer, T = 768 45 vs 33)
// ... while the workgroup stays within 16 waves and its merge slabs within the 64 KB of LDS a launch gets by default
inline bool prefill16_pair_fits(int G, int64_t d, int tt, const AttnPrefillTune &tune) {
    return tune.pf_ksplit >= 2 && G * tt * 2 <= 16 && prefill16_slab_bytes(G, d, tt) <= kPfDefaultLds;
}

// LDS tiles in the ring (FL_ATTN_PF_STAGES, 2..4).  Measured: a deeper ring buys nothing -- Mistral T = 512 25 / 26 /
// 25 us per layer with 2 / 3 / 4 tiles, T = 768 41 / 40 / 42: with one wave per SIMD a key step is a chain of
// dependent LDS read -> MFMA -> shuffle -> exp -> MFMA latencies (~1.5 us), not a wait for the tile.
// ks == 2: two stages of two tiles, the merge slabs in the tiles' place.
inline Prefill16Launch prefill16_launch(int G, int64_t d, int TT, int ks, const AttnPrefillTune &tune) {
    Prefill16Launch l;
    l.nst = ks == 2 ? 2 : std::max(2, std::min(4, G * TT <= 8 ? tune.pf_stages : 2));
    l.lds = std::max((size_t)l.nst * ks * kPfTileBytes32 * (size_t)d, ks == 2 ? prefill16_slab_bytes(G, d, TT) : (size_t)0);
    l.block = G * TT * ks * 64;
    return l;
}

// ------------------------------------------------------------------------------- one prompt
struct AttnPrefillPlan {
    int rows;                           // 16: attn_prefill_mfma_kernel<d, ks>; 32: attn_prefill32_kernel<d, nw, ksf>
    int nw, ksf, TB, paired, gsub;      // 32 rows: waves per workgroup, waves per (head, token block), 32-token blocks per workgroup,
    const char *tag;                    //          work distribution (0 plain, 1 paired, 2 snake), heads per subgroup (0: all G)
    int TT, ks, nst;                    // 16 rows: token sub-tiles per workgroup, key split, ring depth
    unsigned grid_x, grid_y;
    int block;
    size_t lds;
};

// force: 0 automatic, 2 the 16-row kernel, 3 the 32-row kernel (fl_op_attention pins one; the 32-row kernel needs scale > 0: its
// row maximum is taken before the scale is applied).  cus: the CUs of the current device, the snake grid.
inline AttnPrefillPlan plan_attn_prefill(int64_t T, int64_t H, int64_t Hkv, int64_t d, int force, bool scale_positive, int cus,
                                         const AttnPrefillTune &tune) {
    AttnPrefillPlan p{};
    const int G = (int)(H / Hkv);
    const bool g124 = G == 1 || G == 2 || G == 4;
    const int pf32_min_t = tune.pf32_min_t > 0 ? tune.pf32_min_t : (g124 ? kPf32MinT124 : (G > 4 ? kPf32MinTWide : kPf32MinTOther));
    const bool gap = tune.pf32_min_t <= 0 && g124 && T > kPf32FourWaveMaxT && T < kPf32PairMinT;
    if ((force == 3 || (force == 0 && T >= pf32_min_t && !gap)) && scale_positive) {
        // waves per workgroup: 8 (G = 1, 2, 4), 6 (G = 3), else G.  4-wave workgroups (half the K/V reuse, one wave per SIMD) lost
        // everywhere: T = 2048 105 / 180 us, T = 4096 371 / 515.
        const int NW = G <= 4 ? (8 / G) * G : G;
        int TB = NW / G;
        // too few (block, kv head) items to balance: halve the token blocks and split every block's keys over a wave pair
        const int ks2_mode = tune.pf32_ks2;
        bool ks2 = NW == 8 && TB % 2 == 0 && (ks2_mode >= 0 ? ks2_mode != 0 : ((T + 32 * TB - 1) / (32 * TB)) * Hkv < kPfTwoRounds);
        // groups of 5..8 heads: wave pairs only fit when the group is dealt in subgroups of four heads (8 waves = 4 heads x a pair)
        int gsub = 0;
        if (!ks2 && G > 4 && (ks2_mode >= 0 ? ks2_mode != 0 : ((T + 31) / 32) * Hkv < kPfTwoRounds)) { ks2 = true; gsub = 4; TB = 2; }
        if (ks2) TB /= 2;
        // ... and when even the wave pairs leave fewer than two rounds of items: FOUR waves per (head, block), groups of four or more
        // heads dealt two heads at a time -- twice the items again, the longest block's chain a quarter (attn_pf32_ks2 = 4 forces it)
        int ksf = ks2 ? 2 : 1;
        if (ks2 && G != 3) {
            const int64_t items2 = ((T + 32 * TB - 1) / (32 * TB)) * Hkv * (gsub ? (G + gsub - 1) / gsub : 1);
            // Whole prefills, wave pairs / four waves: Mistral-7B 384 / 512 tokens x 0.994 / 0.988 (against the 16-row kernel it replaces
            // there), 600-1536 a tie, 2048 x 1.019; Qwen2-7B 257-512 x 0.986-0.993, 640-1024 a tie; TinyLlama 300 / 512 x 0.986 / 0.972,
            // 640 a tie: on up to 576 tokens.  (Per launch at 512 tokens, Mistral-7B: 16-row kernel 18.6 us, wave pairs 19.2, four waves 15.6.)
            if (ks2_mode == 4 || (ks2_mode < 0 && items2 < kPfTwoRounds && T <= kPf32FourWaveMaxT)) {
                ksf = 4;
                gsub = G >= 4 ? 2 : 0;
                TB = 8 / (gsub ? gsub : G) / 4;
            }
        }
        const int64_t nb = (T + 32 * TB - 1) / (32 * TB);
        const int64_t nhs = Hkv * (gsub ? (G + gsub - 1) / gsub : 1);
        // two rounds or more of (block, kv head) items: persistent workgroups, one per CU, snake order
        p.paired = tune.pf32_paired >= 0 ? tune.pf32_paired : (nb * nhs >= kPfTwoRounds ? 2 : ((nb + 1) / 2 * nhs >= kPf32PairedMinWgs ? 1 : 0));
        p.rows = 32; p.nw = ksf > 1 ? 8 : NW; p.ksf = ksf; p.TB = TB; p.gsub = gsub;
        p.tag = ksf == 4 ? "32row,ks4" : ksf == 2 ? "32row,ks2" : "32row";
        p.grid_x = (unsigned)(p.paired ? (nb + 1) / 2 : nb); p.grid_y = (unsigned)nhs;
        if (p.paired == 2) { p.grid_x = (unsigned)cus; p.grid_y = 1; }
        p.block = p.nw * 64;
        p.lds = (ksf == 4 ? 2 : 3) * kPfTileBytes32 * (size_t)d * ksf;      // a ring of three steps of ksf tiles (ksf = 4: two)
        return p;
    }
    // token sub-tiles per workgroup: every staged K/V tile then serves TT x G x 16 query rows.  Measured: G = 4
    // (Mistral, T = 2048) 4.75 ms with 4 waves, 4.25 with 8, 4.06 with 16; G = 7 (Qwen2, T = 4096) 10.8 ms with 7
    // waves, 12.3 with 14 (126 VGPRs: 16 waves per CU either way, and a longer token block is more lopsided under
    // the causal mask)
    // ... but only while the grid still covers the chip: at T = 512 (Mistral) 4-wave workgroups (256 of them) take
    // 26 us per layer against 36 us for 64 16-wave ones; at T = 1024 8 waves 49 us against 57 (4) and 67 (16)
    int TT = tune.pf_waves > 0 ? std::max(1, std::min(16, tune.pf_waves) / G) : (G <= 4 ? 16 / G : 1);
    if (tune.pf_waves <= 0)
        while (TT > 1 && ((T + 16 * TT - 1) / (16 * TT)) * Hkv < kPfChipCus) TT >>= 1;
    p.rows = 16; p.TT = TT; p.ks = prefill16_pair_fits(G, d, TT, tune) ? 2 : 1;
    const Prefill16Launch l = prefill16_launch(G, d, TT, p.ks, tune);
    p.nst = l.nst; p.lds = l.lds; p.block = l.block;
    p.grid_x = (unsigned)((T + 16 * TT - 1) / (16 * TT)); p.grid_y = (unsigned)Hkv;
    return p;
}

// ------------------------------------------------------------------------------- a pack of prompts
struct AttnPackedPlan { int TT, ks; };

// Token sub-tiles per workgroup and the key split.  ks: the wave pairs of the 16-row kernel wherever ONE sub-tile's pairs and merge
// slabs fit (its own rule at TT = 1, what a single short prompt gets) -- a function of the head shape alone, so that a member's
// arithmetic never depends on the pack.  TT: as the single prompt's plan picks it (every staged tile then serves TT x G x 16 query
// rows), within what ks allows, halved while the items do not cover the chip or while half the sub-tiles still hold the longest
// member.  counts: the new tokens of the members the launch serves.
inline AttnPackedPlan plan_attn_prefill_packed(int64_t H, int64_t Hkv, int64_t d, const int *counts, int n, const AttnPrefillTune &tune) {
    const int G = (int)(H / Hkv);
    if (tune.pf_waves > 0) {
        const int tt = std::max(1, std::min(16, tune.pf_waves) / G);
        return {tt, prefill16_pair_fits(G, d, tt, tune) ? 2 : 1};
    }
    const int ks = prefill16_pair_fits(G, d, 1, tune) ? 2 : 1;
    int TT = G <= 4 ? 16 / G : 1;
    while (ks == 2 && TT > 1 && !prefill16_pair_fits(G, d, TT, tune)) TT >>= 1;
    int longest = 0;
    for (int s = 0; s < n; s++) longest = std::max(longest, counts[s]);
    auto items = [&](int tt) { int64_t k = 0; for (int s = 0; s < n; s++) k += (counts[s] + 16 * tt - 1) / (16 * tt); return k; };
    while (TT > 1 && (items(TT) * Hkv < kPfChipCus || 16 * (TT >> 1) >= longest)) TT >>= 1;
    return {TT, ks};
}

}  // namespace fl
