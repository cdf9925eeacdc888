// k_prefill_packed.hip -- the two kernels of a packed prefill (fl_batch_prefill): several prompts of one model in ONE forward.
// The rows of every [T_total][..] activation buffer are the prompts' tokens back to back; row r belongs to sequence rows[r].seq and
// is its token rows[r].t.  Everything row-wise (embedding, norms, projections) runs on the packed rows as on one prompt; the two
// kernels here are the places where a row meets its OWN cache: RoPE + KV append, and the causal attention over that cache.
// Both read a small device table the host builds per call (PackedTable, kernels.h).  No kernel waits for another workgroup, there
// are no tickets, spins or atomics, and no sum is ever formed over rows of two sequences: a sequence's output rows depend on that
// sequence alone, whatever else the pack holds and wherever in the pack it sits.
#include "attn_prefill16.h"
#include "attn_prefill_plan.h"
#include "kernels.h"

#include <algorithm>

namespace fl {

// ------------------------------------------------------------------------------- RoPE + KV append
// rope_kv_load / rope_kv_store (common.h), the body of rope_kv_kernel and rope_kv_batch_kernel too, on row r of the pack: RoPE at
// st->pos + t of the row's sequence; q goes to the packed [T_total][H*d] buffer, k and v to slot st->len + t of the row's own cache
// (layer offset kv_layer_off * seq_alloc of that sequence, V transposed or row-major as the sequence's cache is laid out).
template <typename CT>
__global__ __launch_bounds__(256) void rope_kv_packed_kernel(const float *__restrict__ qkv, const PackedTable tb,
                                                             const float *__restrict__ cos_tab, const float *__restrict__ sin_tab,
                                                             int max_pos, CT *__restrict__ q_out, size_t kv_layer_off, int T_total,
                                                             int H, int Hkv, int d, int n_slab, const float *__restrict__ bias) {
    RopeKvPair p;
    if (!rope_kv_load(qkv, (long long)blockIdx.x * 256 + threadIdx.x, T_total, H, Hkv, d, n_slab, bias, p)) return;
    const PackedRow row = tb.rows[p.r];
    const SeqRef &sq = tb.seqs[row.seq];
    const size_t sa = (size_t)sq.seq_alloc;
    const RopeKvDst dst{q_out + (size_t)p.r * H * d, &sq.k, &sq.v, kv_layer_off * sa, sa, &tb.seq_vt[row.seq]};
    rope_kv_store<CT>(p, sq.st->pos + (uint32_t)row.t, sq.st->len + (uint32_t)row.t, cos_tab, sin_tab, max_pos, H, Hkv, d, dst);
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
// prefill16_body (attn_prefill16.h), the body of attn_prefill_mfma_kernel (k_attn_mfma.hip) too, with the workgroup's sequence looked
// up instead of passed in: grid (items, Hkv); item = 16 * TT consecutive tokens of ONE sequence, starting at its token t0 (a multiple
// of 16 * TT); T, len, call0 (== len: a packed call is never chunked), the cache bases and seq_alloc come from the item's SeqRef.
// KS == 2 is the wave-pair key split a single short prompt runs, so a packed member gets the arithmetic -- and at TT = 1, where the
// single prompt's alternation starts at the same tile, the bits -- of its single forward.  Here the pair's alternation is counted from
// the WAVE's own first useful tile (OWN_ORIGIN): the tiles a wave computes on, their order and their split over the pair depend on
// its own 16 tokens, its sequence's lengths and the head shape only -- not on TT, the ring depth or the rest of the pack.
// FULL: the unmasked instantiations (attn_prefill16.h) -- items, TT, ks and the launch geometry are the causal plan's.
template <int D, int KS, bool FULL = false>
__global__ __launch_bounds__(1024) void attn_prefill_packed_mfma_kernel(const bf16_t *__restrict__ q, const PackedTable tb, size_t kv_layer_off,
                                                                       bf16_t *__restrict__ out, int H, int Hkv, float scale, int window,
                                                                       int TT, int nst) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];      // nst x KS x (K tile | V^T tile)
    const int hk = blockIdx.y;
    const PackedItem item = tb.items[blockIdx.x];
    const SeqRef &sq = tb.seqs[item.seq];
    const size_t row0 = (size_t)tb.seq_off[item.seq];            // the sequence's first row in the packed buffers
    const int seq_alloc = __builtin_amdgcn_readfirstlane(sq.seq_alloc);      // (everything of the item is wave-uniform)
    const size_t layer = kv_layer_off * (size_t)seq_alloc;
    const Prefill16Seq v{q + row0 * H * D, reinterpret_cast<const bf16_t *>(sq.k) + layer + (size_t)hk * seq_alloc * D,
                         reinterpret_cast<const bf16_t *>(sq.v) + layer + (size_t)hk * D * seq_alloc, out + row0 * H * D,
                         __builtin_amdgcn_readfirstlane(tb.seq_cnt[item.seq]), __builtin_amdgcn_readfirstlane((int)sq.st->len),
                         __builtin_amdgcn_readfirstlane((int)sq.st->call0), seq_alloc, __builtin_amdgcn_readfirstlane(item.t0)};
    prefill16_body<D, KS, true, FULL>(v, hk, H, Hkv, scale, window, TT, nst, lds);
}

PackedTable PackedHost::at(const void *dev_base) const {
    const unsigned char *b = reinterpret_cast<const unsigned char *>(dev_base);
    PackedTable t;
    t.seqs = reinterpret_cast<const SeqRef *>(b + off_seqs); t.rows = reinterpret_cast<const PackedRow *>(b + off_rows);
    t.items = reinterpret_cast<const PackedItem *>(b + off_items); t.seq_off = reinterpret_cast<const int *>(b + off_off);
    t.seq_cnt = reinterpret_cast<const int *>(b + off_cnt); t.seq_vt = reinterpret_cast<const int *>(b + off_vt);
    return t;
}

void packed_table_build(const SeqRef *refs, const int *counts, const int *vt, int n, int64_t H, int64_t Hkv, int64_t d, PackedHost *out,
                        int pad_rows) {
    PackedHost &p = *out;
    std::vector<int> mfma_counts;
    for (int s = 0; s < n; s++) if (vt[s]) mfma_counts.push_back(counts[s]);
    p.n_seq = n;
    p.TT = 1; p.ks = 1;
    if (!mfma_counts.empty()) {
        const AttnPackedPlan g = plan_attn_prefill_packed(H, Hkv, d, mfma_counts.data(), (int)mfma_counts.size(), attn_prefill_tune());
        p.TT = g.TT; p.ks = g.ks;
    }
    std::vector<PackedRow> rows;
    std::vector<PackedItem> items;
    std::vector<int> off((size_t)n);
    for (int s = 0; s < n; s++) {
        off[(size_t)s] = (int)rows.size();
        for (int t = 0; t < counts[s]; t++) rows.push_back(PackedRow{s, t});
        if (vt[s]) for (int t0 = 0; t0 < counts[s]; t0 += 16 * p.TT) items.push_back(PackedItem{s, t0});
    }
    p.T_total = (int)rows.size(); p.n_items = (int)items.size();
    for (int r = 0; r < pad_rows && !rows.empty(); r++) rows.push_back(rows[(size_t)p.T_total - 1]);
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
                                    int64_t H, int64_t Hkv, int64_t d, float scale, int64_t window, double flops, int mask) {
    const int G = (int)(H / Hkv);
    if (mask != 0 && mask != 1) FL_FAIL(FL_ERR_BAD_ARGUMENT, "packed mfma attention: mask %d is neither causal (0) nor full (1)", mask);
    if (!attn_mfma_supported(FL_DTYPE_BF16, H, Hkv, d)) FL_FAIL(FL_ERR_UNSUPPORTED, "packed mfma attention: head_dim 64 / 128, at most 8 query heads per kv head");
    if (TT < 1 || (ks != 1 && ks != 2) || G * TT * ks > 16 || (ks == 2 && prefill16_slab_bytes(G, d, TT) > kPfDefaultLds))
        FL_FAIL(FL_ERR_BAD_ARGUMENT, "packed mfma attention: %d x %d x %d waves per workgroup", G, TT, ks);
    // ring depth, LDS and block of the 16-row kernel at this TT: never more LDS than the single prompt takes there
    const Prefill16Launch l = prefill16_launch(G, d, TT, ks, attn_prefill_tune());
    const dim3 grid((unsigned)n_items, (unsigned)Hkv), block((unsigned)l.block);
#define FL_PACKED(DD, KK, FF)                                                                                                              \
    return L.launch(KC_ATTN_PREFILL, 0, flops, attn_prefill_packed_mfma_kernel<DD, KK, FF>, grid, block, l.lds, (const bf16_t *)q, tb, kv_layer_off, \
                    (bf16_t *)out, (int)H, (int)Hkv, scale, (int)window, TT, l.nst);
    if (mask == 1) {
        if (d == 128) { if (ks == 2) { FL_PACKED(128, 2, true) } FL_PACKED(128, 1, true) }
        if (ks == 2) { FL_PACKED(64, 2, true) }
        FL_PACKED(64, 1, true)
    }
    if (d == 128) { if (ks == 2) { FL_PACKED(128, 2, false) } FL_PACKED(128, 1, false) }
    if (ks == 2) { FL_PACKED(64, 2, false) }
    FL_PACKED(64, 1, false)
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
