// k_prefill_packed.hip -- the two kernels of a packed prefill (fl_batch_prefill): several prompts of one model in ONE forward.
// The rows of every [T_total][..] activation buffer are the prompts' tokens back to back; row r belongs to sequence rows[r].seq and
// is its token rows[r].t.  Everything row-wise (embedding, norms, projections) runs on the packed rows as on one prompt; the two
// kernels here are the places where a row meets its OWN cache: RoPE + KV append, and the causal attention over that cache.
// Both read a small device table the host builds per call (PackedTable, kernels.h).  No kernel waits for another workgroup, there
// are no tickets, spins or atomics, and no sum is ever formed over rows of two sequences: a sequence's output rows depend on that
// sequence alone, whatever else the pack holds and wherever in the pack it sits.
#include "attn_mfma.h"
#include "kernels.h"

#include <algorithm>

namespace fl {

// ------------------------------------------------------------------------------- RoPE + KV append
// The arithmetic of rope_kv_kernel / rope_kv_batch_kernel, in their order: the projection's fp32 K slabs summed in slab order, the
// (Qwen2) bias, rotate-half RoPE at st->pos + t, the store in the cache's element type.  q goes to the packed [T_total][H*d] buffer;
// k and v to slot st->len + t of the row's own cache (layer offset kv_layer_off * seq_alloc of that sequence, V transposed or
// row-major as the sequence's cache is laid out).  One thread per (row, head, j < d/2) pair.
template <typename CT>
__global__ __launch_bounds__(256) void rope_kv_packed_kernel(const float *__restrict__ qkv, const PackedTable tb,
                                                             const float *__restrict__ cos_tab, const float *__restrict__ sin_tab,
                                                             int max_pos, CT *__restrict__ q_out, size_t kv_layer_off, int T_total,
                                                             int H, int Hkv, int d, int n_slab, const float *__restrict__ bias) {
    const int half = d >> 1;
    const int nheads = H + 2 * Hkv;
    const int per_t = nheads * half;
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long long)T_total * per_t) return;
    const int r = (int)(idx / per_t), rem = (int)(idx % per_t);
    const int hd = rem / half, j = rem % half;
    const PackedRow row = tb.rows[r];
    const SeqRef &sq = tb.seqs[row.seq];
    const float *src = qkv + (size_t)r * nheads * d + (size_t)hd * d;
    float a = src[j], b = src[j + half];
    for (int s = 1; s < n_slab; s++) {                    // K slices of the projection, summed in slab order
        const float *ss = src + (size_t)s * T_total * nheads * d;
        a += ss[j]; b += ss[j + half];
    }
    if (bias) { a += bias[(size_t)hd * d + j]; b += bias[(size_t)hd * d + j + half]; }
    const uint32_t pos = sq.st->pos + (uint32_t)row.t, slot = sq.st->len + (uint32_t)row.t;
    const size_t sa = (size_t)sq.seq_alloc;
    if (hd < H + Hkv) {
        const uint32_t p = pos < (uint32_t)max_pos ? pos : (uint32_t)max_pos - 1;   // host validates range
        const float c = cos_tab[(size_t)p * half + j], s = sin_tab[(size_t)p * half + j];
        float ra, rb;
        rope_rotate(a, b, c, s, ra, rb);
        CT *o = hd < H ? q_out + ((size_t)r * H + hd) * d
                       : reinterpret_cast<CT *>(sq.k) + kv_layer_off * sa + ((size_t)(hd - H) * sa + slot) * d;
        elem<CT>::st(o + j, ra); elem<CT>::st(o + j + half, rb);
    } else if (tb.seq_vt[row.seq]) {                      // V transposed [Hkv][d][seq_alloc]: the MFMA attention layout
        CT *o = reinterpret_cast<CT *>(sq.v) + kv_layer_off * sa + (size_t)(hd - H - Hkv) * d * sa + slot;
        elem<CT>::st(o + (size_t)j * sa, a); elem<CT>::st(o + (size_t)(j + half) * sa, b);
    } else {                                              // V [Hkv][seq_alloc][d]
        CT *o = reinterpret_cast<CT *>(sq.v) + kv_layer_off * sa + ((size_t)(hd - H - Hkv) * sa + slot) * d;
        elem<CT>::st(o + j, a); elem<CT>::st(o + j + half, b);
    }
}

int launch_rope_kv_packed(Launcher &L, int dtype, const float *qkv, const PackedTable &tb, const float *cos_tab, const float *sin_tab,
                          int64_t max_pos, void *q_out, size_t kv_layer_off, int64_t T_total, int64_t H, int64_t Hkv, int64_t d, int n_slab,
                          const float *bias) {
    const int64_t total = T_total * (H + 2 * Hkv) * (d / 2);
    const dim3 grid((unsigned)((total + 255) / 256));
    // algorithmic bytes: the fp32 slabs in, every element out once in the compute dtype
    const double bytes = (double)T_total * (H + 2 * Hkv) * d * (4.0 * n_slab + (dtype == FL_DTYPE_F32 ? 4 : 2));
    if (dtype == FL_DTYPE_F32)
        return L.launch(KC_ROPE_KV, bytes, 0, rope_kv_packed_kernel<float>, grid, dim3(256), 0, qkv, tb, cos_tab, sin_tab, (int)max_pos,
                        (float *)q_out, kv_layer_off, (int)T_total, (int)H, (int)Hkv, (int)d, n_slab, bias);
    return L.launch(KC_ROPE_KV, bytes, 0, rope_kv_packed_kernel<bf16_t>, grid, dim3(256), 0, qkv, tb, cos_tab, sin_tab, (int)max_pos,
                    (bf16_t *)q_out, kv_layer_off, (int)T_total, (int)H, (int)Hkv, (int)d, n_slab, bias);
}

// ------------------------------------------------------------------------------- ragged causal attention
// attn_prefill_mfma_kernel (k_attn_mfma.hip) with the workgroup's sequence looked up instead of passed in:
// grid (items, Hkv); item = 16 * TT consecutive tokens of ONE sequence, starting at its token t0 (a multiple of 16 * TT); workgroup =
// G * TT waves, wave w serving query head w % G for the 16 tokens of sub-tile w / G.  The sequence's K / V^T tiles of 32 keys go
// through the LDS ring by LDS-DMA once per workgroup; len, call0, the cache bases and seq_alloc come from the item's SeqRef.
// Columns past the sequence's end carry q = 0 and are not stored.  A wave skips the tiles wholly outside its own visible range
// (wstart / wend), staging is never skipped.
// KS == 2: the wave-pair key split of the 16-row kernel, which is what a single short prompt runs (FL_ATTN_PF_KSPLIT): two waves per
// (head, sub-tile) take alternate key tiles and merge through LDS at the end, so a packed member gets the arithmetic -- and the bits
// -- of its single forward.  Which of the pair takes a tile is counted from the WAVE's own first useful tile (wstart), not from the
// workgroup's first staged tile.
// Either way the tiles a wave computes on, their order and their split over the pair depend on its own 16 tokens, its sequence's
// lengths and the head shape only -- not on TT, the ring depth or the rest of the pack.
template <int D, int KS>
__global__ __launch_bounds__(1024) void attn_prefill_packed_mfma_kernel(const bf16_t *__restrict__ q, const PackedTable tb, size_t kv_layer_off,
                                                                       bf16_t *__restrict__ out, int H, int Hkv, float scale, int window,
                                                                       int TT, int nst) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];      // nst x (K tile | V^T tile)
    constexpr int TILE = 2 * 32 * D * 2;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), nwv = blockDim.x >> 6;
    const int i = lane & 15, g4 = lane >> 4;
    const int G = H / Hkv, hk = blockIdx.y;
    const PackedItem item = tb.items[blockIdx.x];
    const SeqRef &sq = tb.seqs[item.seq];
    const int T = __builtin_amdgcn_readfirstlane(tb.seq_cnt[item.seq]);   // the sequence's new tokens (everything of the item is wave-uniform)
    const size_t row0 = (size_t)tb.seq_off[item.seq];            // ... and its first row in the packed buffers
    q += row0 * H * D; out += row0 * H * D;                      // (from here on q / out are the sequence's own rows)
    const int seq_alloc = __builtin_amdgcn_readfirstlane(sq.seq_alloc);
    const int wq = wave % (G * TT), half = wave / (G * TT);      // (half: KS == 2 only)
    const int hq = hk * G + wq % G;
    const int tb0 = __builtin_amdgcn_readfirstlane(item.t0);     // first token of the workgroup
    const int t0 = tb0 + (wq / G) * 16;                          // first token of this wave
    const int len = __builtin_amdgcn_readfirstlane((int)sq.st->len);
    const int t = t0 + i;                                        // this lane's column
    const bool col_ok = t < T;

    bf16x8 qf[D / 32];
#pragma unroll
    for (int dk = 0; dk < D / 32; dk++) {
        if (col_ok) qf[dk] = ld_bf16x8(q + ((size_t)t * H + hq) * D + dk * 32 + g4 * 8);
        else {
#pragma unroll
            for (int j = 0; j < 8; j++) qf[dk][j] = (__bf16)0.f;
        }
    }
    // the keys cached before the call are an unmasked prefix (call0 == len: a packed call is never chunked); the causal +
    // sliding-window mask runs over the sequence's own new tokens
    const int c0 = __builtin_amdgcn_readfirstlane((int)sq.st->call0);
    int lo = c0;
    if (window >= 0 && len + t - window > c0) lo = len + t - window;
    const int lo_q = col_ok ? lo : 0, hi_q = col_ok ? len + t + 1 : 0;
    const int pre_hi = col_ok ? c0 : 0;
    int wstart = 0;
    if (c0 == 0 && window >= 0 && len + t0 - window > 0) wstart = ((len + t0 - window) / 32) * 32;
    const int wend = t0 < T ? len + min(T, t0 + 16) : 0;

    MfmaAttnState<D> s; s.init();
    const bf16_t *kb = reinterpret_cast<const bf16_t *>(sq.k) + kv_layer_off * (size_t)seq_alloc + (size_t)hk * seq_alloc * D;
    const bf16_t *vb = reinterpret_cast<const bf16_t *>(sq.v) + kv_layer_off * (size_t)seq_alloc + (size_t)hk * D * seq_alloc;
    int kstart = 0;
    if (c0 == 0 && window >= 0 && len + tb0 - window > 0) kstart = ((len + tb0 - window) / 32) * 32;
    const int kend = len + min(T, tb0 + 16 * TT);                // <= the cache's capacity <= seq_alloc (a multiple of 32)
    const int nsteps = (kend - kstart + 31) / 32;
    constexpr int NI = D / 16 + D / 16;
    const int per = (NI + nwv - 1) / nwv;
    if constexpr (KS == 2) {
        // super-steps of two tiles (buffers [stage][tile]); one barrier per super-step, two LDS stages
        const int nsuper = (nsteps + 1) / 2;
        const int mine = half ^ (((max(wstart, kstart) - kstart) >> 5) & 1);     // this wave's tile of every super-step
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
        // merge the two key halves through LDS (the tiles are dead after the barrier), as the 16-row kernel does
        __syncthreads();
        float *slab = reinterpret_cast<float *>(lds) + (size_t)wq * (16 * D + 32);
        float lt1 = s.l;
        lt1 += __shfl_xor(lt1, 16, 64);
        lt1 += __shfl_xor(lt1, 32, 64);
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
            const int tt = t0 + qq;
            if (tt < T) {
                const float inv = 1.0f / lr;
                bf16_t *o = out + ((size_t)tt * H + hq) * D;
#pragma unroll
                for (int db = 0; db < D / 16; db++)
                    o[db * 16 + i] = float_to_bf16_bits((s.O[db][r] * a0 + slab[qq * D + db * 16 + i] * a1) * inv);
            }
        }
        return;
    } else {
        // the plain ring of nst tiles, nst - 1 of them in flight
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

        float lt = s.l;
        lt += __shfl_xor(lt, 16, 64);
        lt += __shfl_xor(lt, 32, 64);
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int qq = 4 * g4 + r;
            const float lr = __shfl(lt, qq, 64);
            const int tt = t0 + qq;
            if (tt < T) {
                const float inv = 1.0f / lr;
                bf16_t *o = out + ((size_t)tt * H + hq) * D;
#pragma unroll
                for (int db = 0; db < D / 16; db++) o[db * 16 + i] = float_to_bf16_bits(s.O[db][r] * inv);
            }
        }
    }
}

// Token sub-tiles per workgroup and the key split.  ks: the wave pairs of the 16-row kernel wherever ONE sub-tile's pairs and merge
// slabs fit (its own rule at TT = 1, what a single short prompt gets) -- a function of the head shape alone, so that a member's
// arithmetic never depends on the pack.  TT: as the 16-row kernel picks it (every staged tile then serves TT x G x 16 query rows),
// within what ks allows, halved while the items do not cover the chip or while half the sub-tiles still hold the longest member.
// counts: the new tokens of the members the launch serves.
void attn_packed_geometry(int64_t H, int64_t Hkv, int64_t d, const int *counts, int n, int *TT_out, int *ks_out) {
    const int G = (int)(H / Hkv);
    const int tt_waves = tune(TK_ATTN_PF_WAVES);
    auto fits2 = [&](int tt) { return tune(TK_ATTN_PF_KSPLIT) >= 2 && G * tt * 2 <= 16 && (size_t)G * tt * (16 * d + 32) * 4 <= 64 * 1024; };
    if (tt_waves > 0) {
        *TT_out = std::max(1, std::min(16, tt_waves) / G);
        *ks_out = fits2(*TT_out) ? 2 : 1;
        return;
    }
    const int ks = fits2(1) ? 2 : 1;
    int TT = G <= 4 ? 16 / G : 1;
    while (ks == 2 && TT > 1 && !fits2(TT)) TT >>= 1;
    int longest = 0;
    for (int s = 0; s < n; s++) longest = std::max(longest, counts[s]);
    auto items = [&](int tt) { int64_t k = 0; for (int s = 0; s < n; s++) k += (counts[s] + 16 * tt - 1) / (16 * tt); return k; };
    while (TT > 1 && (items(TT) * Hkv < 256 || 16 * (TT >> 1) >= longest)) TT >>= 1;
    *TT_out = TT; *ks_out = ks;
}

PackedTable PackedHost::at(const void *dev_base) const {
    const unsigned char *b = reinterpret_cast<const unsigned char *>(dev_base);
    PackedTable t;
    t.seqs = reinterpret_cast<const SeqRef *>(b + off_seqs); t.rows = reinterpret_cast<const PackedRow *>(b + off_rows);
    t.items = reinterpret_cast<const PackedItem *>(b + off_items); t.seq_off = reinterpret_cast<const int *>(b + off_off);
    t.seq_cnt = reinterpret_cast<const int *>(b + off_cnt); t.seq_vt = reinterpret_cast<const int *>(b + off_vt);
    return t;
}

void packed_table_build(const SeqRef *refs, const int *counts, const int *vt, int n, int64_t H, int64_t Hkv, int64_t d, PackedHost *out) {
    PackedHost &p = *out;
    std::vector<int> mfma_counts;
    for (int s = 0; s < n; s++) if (vt[s]) mfma_counts.push_back(counts[s]);
    p.n_seq = n;
    p.TT = 1; p.ks = 1;
    if (!mfma_counts.empty()) attn_packed_geometry(H, Hkv, d, mfma_counts.data(), (int)mfma_counts.size(), &p.TT, &p.ks);
    std::vector<PackedRow> rows;
    std::vector<PackedItem> items;
    std::vector<int> off((size_t)n);
    for (int s = 0; s < n; s++) {
        off[(size_t)s] = (int)rows.size();
        for (int t = 0; t < counts[s]; t++) rows.push_back(PackedRow{s, t});
        if (vt[s]) for (int t0 = 0; t0 < counts[s]; t0 += 16 * p.TT) items.push_back(PackedItem{s, t0});
    }
    p.T_total = (int)rows.size(); p.n_items = (int)items.size();
    p.off_seqs = 0;
    p.off_rows = sizeof(SeqRef) * (size_t)n;
    p.off_items = p.off_rows + sizeof(PackedRow) * rows.size();
    p.off_off = p.off_items + sizeof(PackedItem) * items.size();
    p.off_cnt = p.off_off + 4 * (size_t)n;
    p.off_vt = p.off_cnt + 4 * (size_t)n;
    p.bytes.assign(p.off_vt + 4 * (size_t)n, 0);
    memcpy(p.bytes.data() + p.off_seqs, refs, sizeof(SeqRef) * (size_t)n);
    memcpy(p.bytes.data() + p.off_rows, rows.data(), sizeof(PackedRow) * rows.size());
    if (!items.empty()) memcpy(p.bytes.data() + p.off_items, items.data(), sizeof(PackedItem) * items.size());
    memcpy(p.bytes.data() + p.off_off, off.data(), 4 * (size_t)n);
    memcpy(p.bytes.data() + p.off_cnt, counts, 4 * (size_t)n);
    memcpy(p.bytes.data() + p.off_vt, vt, 4 * (size_t)n);
}

int launch_attn_prefill_packed_mfma(Launcher &L, const void *q, const PackedTable &tb, int n_items, int TT, int ks, size_t kv_layer_off, void *out,
                                    int64_t H, int64_t Hkv, int64_t d, float scale, int64_t window, double flops) {
    const int G = (int)(H / Hkv);
    if (!attn_mfma_supported(FL_DTYPE_BF16, H, Hkv, d)) FL_FAIL(FL_ERR_UNSUPPORTED, "packed mfma attention: head_dim 64 / 128, at most 8 query heads per kv head");
    const size_t slabs = (size_t)G * TT * (16 * d + 32) * 4;     // ks == 2: the merge slabs, in the tiles' place
    if (TT < 1 || (ks != 1 && ks != 2) || G * TT * ks > 16 || (ks == 2 && slabs > 64 * 1024))
        FL_FAIL(FL_ERR_BAD_ARGUMENT, "packed mfma attention: %d x %d x %d waves per workgroup", G, TT, ks);
    const dim3 grid((unsigned)n_items, (unsigned)Hkv), block((unsigned)(G * TT * ks * 64));
    // ring depth and LDS of the 16-row kernel at this TT (launch_attn_prefill_mfma): never more LDS than it takes there
    const int nst = ks == 2 ? 2 : std::max(2, std::min(4, G * TT <= 8 ? tune(TK_ATTN_PF_STAGES) : 2));
    const size_t lds = std::max((size_t)nst * ks * (size_t)(2 * 32 * d * 2), ks == 2 ? slabs : (size_t)0);
#define FL_PACKED(DD, KK)                                                                                                                  \
    return L.launch(KC_ATTN_PREFILL, 0, flops, attn_prefill_packed_mfma_kernel<DD, KK>, grid, block, lds, (const bf16_t *)q, tb, kv_layer_off, \
                    (bf16_t *)out, (int)H, (int)Hkv, scale, (int)window, TT, nst);
    if (d == 128) { if (ks == 2) { FL_PACKED(128, 2) } FL_PACKED(128, 1) }
    if (ks == 2) { FL_PACKED(64, 2) }
    FL_PACKED(64, 1)
#undef FL_PACKED
}

// ------------------------------------------------------------------------------- the members' step states
// What set_state_kernel (model.hip) does for one cache, for every member of the call in ONE launch: block s writes sequence s's
// StepState (token, RoPE offset, cached length, call0 = len, step 0, no EOS, done / error cleared) and token selection, and zeroes
// its fused-attention tickets (they restart with the step counter).
__global__ __launch_bounds__(64) void packed_set_states_kernel(const PackedTable tb, const PackedSeqInit *__restrict__ init, int n_tickets) {
    const SeqRef &sq = tb.seqs[blockIdx.x];
    const PackedSeqInit &in = init[blockIdx.x];
    if (threadIdx.x == 0) {
        StepState *st = sq.st;
        st->token = in.token; st->pos = in.pos; st->len = in.len; st->call0 = in.len; st->step = 0; st->eos = -1; st->done = 0; st->error = 0;
        *sq.ss = in.ss;
    }
    for (int l = threadIdx.x; l < n_tickets; l += 64) in.heads_done[l] = 0;
}

int launch_packed_set_states(Launcher &L, const PackedTable &tb, const PackedSeqInit *init_dev, int n_seq, int n_tickets) {
    return L.launch(KC_CONVERT, (double)n_seq * sizeof(PackedSeqInit), 0, packed_set_states_kernel, dim3((unsigned)n_seq), dim3(64), 0, tb, init_dev, n_tickets);
}

// ... and what the host wants back from them after token selection, gathered for one copy: out[2 s] = sequence s's token,
// out[2 s + 1] = its error word
__global__ __launch_bounds__(64) void packed_collect_kernel(const PackedTable tb, uint32_t *__restrict__ out, int n_seq) {
    const int s = blockIdx.x * 64 + threadIdx.x;
    if (s >= n_seq) return;
    const StepState *st = tb.seqs[s].st;
    out[2 * s] = st->token; out[2 * s + 1] = st->error;
}

int launch_packed_collect(Launcher &L, const PackedTable &tb, uint32_t *out_dev, int n_seq) {
    return L.launch(KC_CONVERT, (double)n_seq * 16, 0, packed_collect_kernel, dim3((unsigned)((n_seq + 63) / 64)), dim3(64), 0, tb, out_dev, n_seq);
}

// ------------------------------------------------------------------------------- last rows
// dst[s][:] = src[last row of sequence s][:] for the n_slab slabs of src (fp32, h a multiple of 4): the rows the final norm and
// lm_head run on, gathered to [n_slab][n][h]
__global__ __launch_bounds__(256) void gather_last_rows_kernel(const float *__restrict__ src, const PackedTable tb, float *__restrict__ dst,
                                                               int n_seq, int h, int n_slab, long long src_slab, long long dst_slab) {
    const int s = blockIdx.x, sl = blockIdx.y;
    const size_t r = (size_t)(tb.seq_off[s] + tb.seq_cnt[s] - 1);
    const float *a = src + (size_t)sl * src_slab + r * h;
    float *o = dst + (size_t)sl * dst_slab + (size_t)s * h;
    for (int c = threadIdx.x * 4; c < h; c += 256 * 4) *reinterpret_cast<float4v *>(o + c) = *reinterpret_cast<const float4v *>(a + c);
}

int launch_gather_last_rows(Launcher &L, const float *src, const PackedTable &tb, float *dst, int n_seq, int64_t h, int n_slab, int64_t src_slab,
                            int64_t dst_slab) {
    if (h % 4) FL_FAIL(FL_ERR_UNSUPPORTED, "packed prefill: hidden size %lld is not a multiple of 4", (long long)h);
    return L.launch(KC_CONVERT, (double)n_seq * h * 8 * n_slab, 0, gather_last_rows_kernel, dim3((unsigned)n_seq, (unsigned)n_slab), dim3(256), 0, src,
                    tb, dst, n_seq, (int)h, n_slab, (long long)src_slab, (long long)dst_slab);
}

}  // namespace fl
