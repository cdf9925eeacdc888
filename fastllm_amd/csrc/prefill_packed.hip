// prefill_packed.hip -- fl_batch_prefill: several prompts of one model in ONE forward (model.h: batch_prefill).
// Up to about 128 rows the projections of a prompt are a weight stream, so n short prompts forwarded one after the other read the
// weights n times; packed, their tokens are the rows of one forward.  Everything row-wise runs at T = the total token count through
// the same launches (and the same planner) as a single prompt; RoPE / KV append and attention go through k_prefill_packed.hip, which
// finds every row's own cache in a device table; the final norm, lm_head and token selection run on the n last rows only.
// Eager launches: no graph, no residual or RoPE epilogues in the projections.
#include "model.h"
#include "lookup.h"

#include <algorithm>

namespace fl {

namespace {

// the model's packed buffers for a call of n sequences whose table image takes tab_bytes
int grow_packed(Model *m, Shard &sh, int n, size_t tab_bytes) {
    PackedScratch &ps = sh.packed;
    const Dims &D = m->D;
    if (!ps.host_result) FL_HIP(hipHostMalloc((void **)&ps.host_result, kMaxBatch * 8, hipHostMallocDefault));
    if (ps.tab_bytes < tab_bytes || ps.host_tab_bytes < tab_bytes || ps.cap_n < n) FL_HIP(hipStreamSynchronize(sh.stream));   // (idle anyway: every call ends with a synchronise)
    if (ps.tab_bytes < tab_bytes) {
        if (ps.tab) (void)hipFree(ps.tab);
        ps.tab = nullptr; ps.tab_bytes = 0;
        const size_t cap = (tab_bytes + tab_bytes / 2 + 4095) / 4096 * 4096;
        FL_HIP(hipMalloc(&ps.tab, cap));
        ps.tab_bytes = cap;
    }
    if (ps.host_tab_bytes < tab_bytes) {
        if (ps.host_tab) (void)hipHostFree(ps.host_tab);
        ps.host_tab = nullptr; ps.host_tab_bytes = 0;
        const size_t cap = (tab_bytes + tab_bytes / 2 + 4095) / 4096 * 4096;
        FL_HIP(hipHostMalloc((void **)&ps.host_tab, cap, hipHostMallocDefault));
        ps.host_tab_bytes = cap;
    }
    if (ps.cap_n < n) {
        for (void *p : ps.allocs) (void)hipFree(p);
        ps.allocs.clear(); ps.cap_n = 0;
        const size_t cap = (size_t)std::min(kMaxBatch, std::max(n, 8));
        const size_t nsl = (size_t)std::max(kMaxKSplit, kMaxKSplitMid);
        FL_TRY(dev_alloc(ps.allocs, (void **)&ps.xl, cap * D.h * 4, nullptr));
        FL_TRY(dev_alloc(ps.allocs, (void **)&ps.dl, nsl * cap * D.h * 4, nullptr));
        FL_TRY(dev_alloc(ps.allocs, &ps.xnl, cap * D.h * m->esize(), nullptr));
        FL_TRY(dev_alloc(ps.allocs, (void **)&ps.inv_rms, cap * 4, nullptr));
        FL_TRY(dev_alloc(ps.allocs, (void **)&ps.logits, cap * D.V * 4, nullptr));
        FL_TRY(dev_alloc(ps.allocs, (void **)&ps.result, kMaxBatch * 8, nullptr));
        ps.cap_n = (int)cap;
    }
    return FL_OK;
}

// fl_batch_verify's buffers: the selection block (zeroed ONCE here: the kernel puts its tickets back) and its pinned image, the shared
// [R][V] block scratch, and for a sampled pack the probabilities of one block
int grow_verify(Model *m, Shard &sh, bool any_sampled, float **rows, int64_t *R) {
    PackedScratch &ps = sh.packed;
    if (!ps.verify_out) {
        FL_TRY(dev_alloc(sh.allocs, (void **)&ps.verify_out, (size_t)kVerifyPackedWords * 4, &m->hbm_bytes));
        FL_HIP(hipMemsetAsync(ps.verify_out, 0, (size_t)kVerifyPackedWords * 4, sh.stream));
    }
    if (!ps.host_verify) FL_HIP(hipHostMalloc((void **)&ps.host_verify, (size_t)kVerifyPackedWords * 4, hipHostMallocDefault));
    FL_TRY(score_block_scratch(m, sh, rows, R));
    if (any_sampled && ps.verify_prob_R < *R) {
        const int64_t V = m->D.V;
        FL_HIP(hipStreamSynchronize(sh.stream));                 // (idle anyway: every call ends with a synchronise)
        if (ps.verify_prob) { (void)hipFree(ps.verify_prob); ps.verify_prob = nullptr; }
        m->hbm_bytes -= ps.verify_prob_R * V * 4; ps.verify_prob_R = 0;
        std::vector<void *> own;
        FL_TRY(dev_alloc(own, (void **)&ps.verify_prob, (size_t)(*R * V) * 4, nullptr));
        m->hbm_bytes += *R * V * 4; ps.verify_prob_R = *R;
    }
    return FL_OK;
}

// fl_batch_embed's buffers: the pooled vectors of `rows` outputs and the column chunks' partial sums of squares.  Allocated at a
// model's first embed call and regrown with the largest one; models that never embed pay nothing.
int grow_embed(Model *m, Shard &sh, size_t rows) {
    PackedScratch &ps = sh.packed;
    if (ps.embed_rows >= rows) return FL_OK;
    const size_t h = (size_t)m->D.h, nch = (size_t)pool_rows_chunks(m->D.h);
    FL_HIP(hipStreamSynchronize(sh.stream));                     // (idle anyway: every call ends with a synchronise)
    if (ps.embed_out) { (void)hipFree(ps.embed_out); ps.embed_out = nullptr; }
    if (ps.embed_part) { (void)hipFree(ps.embed_part); ps.embed_part = nullptr; }
    m->hbm_bytes -= (int64_t)(ps.embed_rows * (h + nch) * 4); ps.embed_rows = 0;
    const size_t cap = std::min<size_t>(std::max<size_t>(rows + rows / 2, 64), std::max<size_t>(rows, (size_t)tune(TK_PREFILL_CHUNK)));
    std::vector<void *> own;
    FL_TRY(dev_alloc(own, (void **)&ps.embed_out, cap * h * 4, nullptr));
    FL_TRY(dev_alloc(own, (void **)&ps.embed_part, cap * nch * 4, nullptr));
    m->hbm_bytes += (int64_t)(cap * (h + nch) * 4); ps.embed_rows = cap;
    return FL_OK;
}

// The ticket words of the selection block are zeroed once and put back by the kernel itself.  A call that fails between two lm_head
// blocks, or whose tickets did not come back 0, would leave a straddling member's ticket behind for every later call: unless the call
// ended well, the 64 words are zeroed again on the way out (enqueued ahead of StreamDrain's wait: declare it after the drain).
struct TicketReset {
    uint32_t *out; hipStream_t s; bool armed = true;
    ~TicketReset() { if (armed) (void)hipMemsetAsync(out + kVerifyPackedTicket, 0, (size_t)kMaxBatch * 4, s); }
};

struct StreamDrain {            // an early return leaves nothing in flight that reads the call's host buffers
    hipStream_t s;
    ~StreamDrain() { (void)hipStreamSynchronize(s); }
};

// How a call names itself in its refusals: fl_batch_prefill and fl_batch_score keep the words they always had (and share them: one
// message for one fault), a packed verify and a packed embed say what they are.
struct PackWords { const char *prefix, *noun; };
constexpr PackWords kWordsPrefill{"", "packed prefill"}, kWordsVerify{"fl_batch_verify: ", "packed verify"}, kWordsEmbed{"fl_batch_embed: ", "packed embed"};

// What a pack must look like whoever forwards it, decided without the model or a cache being looked at: n, the offsets, at most
// max_rows rows per member (0: any), no null cache, no cache twice.
int check_pack_shape(const PackWords &w, Cache *const *caches, size_t n, const size_t *offsets, size_t max_rows) {
    if (n < 1 || n > (size_t)kMaxBatch) FL_FAIL(FL_ERR_BAD_ARGUMENT, "%s%zu sequences: a %s takes 1..%d", w.prefix, n, w.noun, kMaxBatch);
    if (offsets[0] != 0) FL_FAIL(FL_ERR_BAD_ARGUMENT, "%soffsets[0] is %zu, not 0", w.prefix, offsets[0]);
    for (size_t i = 0; i < n; i++) {
        if (offsets[i + 1] <= offsets[i]) FL_FAIL(FL_ERR_BAD_ARGUMENT, "%ssequence %zu is empty (offsets must increase)", w.prefix, i);
        if (max_rows && offsets[i + 1] - offsets[i] > max_rows)
            FL_FAIL(FL_ERR_BAD_ARGUMENT, "%ssequence %zu has %zu rows, n_draft exceeds FL_VERIFY_MAX_DRAFT (%d)", w.prefix, i, offsets[i + 1] - offsets[i], FL_VERIFY_MAX_DRAFT);
        if (!caches[i]) FL_FAIL(FL_ERR_BAD_ARGUMENT, "%scache %zu is null or belongs to another model", w.prefix, i);
        for (size_t j = 0; j < i; j++) if (caches[j] == caches[i]) FL_FAIL(FL_ERR_BAD_ARGUMENT, "%scache %zu appears twice in the call", w.prefix, i);
    }
    return FL_OK;
}

// what a packed verify step hands back: member i's ids at tokens_out[offsets[i] ..], n_out[i] of them
struct VerifyMode { uint32_t *tokens_out; size_t *n_out; };

// batch_prefill, or -- score != null -- batch_score, or -- vf != null -- batch_verify: the same checks and the same layers; behind them
// either the n last rows go through the final norm, lm_head and token selection, or ALL rows go through the final norm and lm_head in
// blocks, each scored (model.h: ScoreCall) or each selected and scanned per member (launch_verify_packed); or -- emb != null --
// batch_embed: the layers under emb->mask, the final norm on all rows and the pool launch (k_pool.hip): no lm_head, no selection
int packed_forward(Model *m, Cache *const *caches, size_t n, const uint32_t *ids, const size_t *offsets, const size_t *pos,
                   const fl_sampler *samplers, uint32_t *tokens_out, float *logits_out, const fl_score *score, const VerifyMode *vf = nullptr,
                   const fl_embed *emb = nullptr, float *emb_out = nullptr) {
    // ---- everything that can be refused is refused here, before the device or any cache is touched
    const PackWords &w = vf ? kWordsVerify : emb ? kWordsEmbed : kWordsPrefill;
    if (!m || !caches || !ids || !offsets || !pos) FL_FAIL(FL_ERR_BAD_ARGUMENT, "null argument");
    if (n < 1 || n > (size_t)kMaxBatch) FL_FAIL(FL_ERR_BAD_ARGUMENT, "%s%zu sequences: a %s takes 1..%d", w.prefix, n, w.noun, kMaxBatch);
    if (m->tp > 1 || m->shards.size() != 1) FL_FAIL(FL_ERR_UNSUPPORTED, "%sa %s runs on one GPU (tp_size %d)", w.prefix, w.noun, m->tp);
    FL_TRY(check_pack_shape(w, caches, n, offsets, vf ? (size_t)FL_VERIFY_MAX_DRAFT + 1 : 0));
    for (size_t i = 0; i < n; i++) {
        if (caches[i]->m != m) FL_FAIL(FL_ERR_BAD_ARGUMENT, "%scache %zu is null or belongs to another model", w.prefix, i);
        if (tokens_out) FL_TRY(refuse_logit_rules(caches[i], "fl_batch_prefill with tokens_out"));   // (its selection reads the raw rows)
        if (tokens_out) FL_TRY(refuse_guide(caches[i], "fl_batch_prefill with tokens_out"));
        if (vf) FL_TRY(refuse_logit_rules(caches[i], "fl_batch_verify"));
        if (vf) FL_TRY(refuse_guide(caches[i], "fl_batch_verify"));
    }
    if (emb) FL_TRY(check_embed(emb, m->D.h));
    const int mask = emb ? emb->mask : FL_MASK_CAUSAL;
    if (mask == FL_MASK_FULL)
        for (size_t i = 0; i < n; i++)
            if (caches[i]->len != 0)
                FL_FAIL(FL_ERR_UNSUPPORTED, "fl_batch_embed: FL_MASK_FULL needs an empty cache, cache %zu holds %zu tokens (a prefix computed causally is not the full-mask model's)", i, caches[i]->len);
    const size_t T_total = offsets[n];
    for (size_t r = 0; r < T_total; r++) FL_TRY(check_token(m, ids[r], "token"));
    const size_t chunk_max = (size_t)tune(TK_PREFILL_CHUNK);
    if (T_total > chunk_max) FL_FAIL(FL_ERR_UNSUPPORTED, "%s%zu tokens in one %s: at most %zu (FL_PREFILL_CHUNK); split the call", w.prefix, T_total, w.noun, chunk_max);
    for (size_t i = 0; i < n; i++) {
        if (vf) FL_TRY(check_verify(m, caches[i], offsets[i + 1] - offsets[i] - 1, pos[i]));      // (a member's rows: its token and its drafts)
        else FL_TRY(check_call(m, caches[i], offsets[i + 1] - offsets[i], pos[i]));
    }
    std::vector<SampleState> sampler(n);
    bool any_sampled = false;
    for (size_t i = 0; i < n; i++) {
        FL_TRY(make_sampler(samplers ? samplers + i : nullptr, m->D.V, &sampler[i]));
        any_sampled |= sampler[i].on != 0;
    }
    std::vector<uint32_t> tg;
    if (score) {
        FL_TRY(check_score(score, T_total, m->D.V));
        // targets NULL: next-token scoring per sequence -- the last row of every member has no target
        tg.assign(T_total, kScoreNoTarget);
        for (size_t i = 0; i < n; i++)
            for (size_t r = offsets[i]; r < offsets[i + 1]; r++)
                if (score->targets) tg[r] = score->targets[r];
                else if (r + 1 < offsets[i + 1]) tg[r] = ids[r + 1];
    }
    debug_inject("batch_prefill");

    const Dims &D = m->D;
    const int dt = m->dtype;
    const size_t es = m->esize();
    std::lock_guard<std::mutex> lock(m->mu);
    Shard &sh = m->shards[0];
    FL_HIP(hipSetDevice(sh.device));
    // A verify pack of ONE row is forwarded as two: the row and a copy of it (the same id, the same table entry, so the same RoPE
    // offset and the same cache slot, written twice with the same values; the copy belongs to no member, is not attended, selected
    // or returned).  The row-wise launches of a one-row forward are the planner's T = 1 kernels, whose sums differ in the last bits
    // from the short-prompt kernels a pack of 2 .. 32 rows runs: with the copy a stream verified alone and the same stream among a
    // few others agree bit for bit.  This removes ONE of the planner's row-count thresholds, the one a batcher crosses whenever a
    // stream is left alone; it does not make a member independent of the pack's size in general (the header says what holds).
    const int64_t pad = vf && T_total == 1 ? 1 : 0;
    const int64_t T = (int64_t)T_total + pad;
    const uint32_t twice[2] = {ids[0], ids[0]};
    if (sh.pre.cap_T < T) FL_TRY(grow_prefill_scratch(m, sh, T));
    Scratch &sc = sh.pre;

    // ---- the call's table: every member's SeqRef, rows, attention items (members in the MFMA layout; the others per sequence below)
    std::vector<SeqRef> refs(n);
    std::vector<int> counts(n), vt(n);
    bool any_mfma = false, any_plain = false;
    double attn_flops = 0;
    for (size_t i = 0; i < n; i++) {
        Cache *c = caches[i];
        CacheShard &cs = c->shards[0];
        refs[i] = SeqRef{cs.st, cs.ss, cs.k, cs.v, cs.part_m, cs.part_l, cs.part_o, cs.counters, cs.out_tokens, cs.sel_scratch, (int)c->seq_alloc, c->nsplit};
        counts[i] = (int)(offsets[i + 1] - offsets[i]);
        vt[i] = c->v_transposed ? 1 : 0;
        (c->v_transposed ? any_mfma : any_plain) = true;
        attn_flops += 4.0 * counts[i] * (double)(c->len + (size_t)counts[i]) * sh.Hs * D.d;
    }
    PackedHost ph;
    packed_table_build(refs.data(), counts.data(), vt.data(), (int)n, sh.Hs, sh.Hkvs, D.d, &ph, (int)pad);
    // ... and behind it every member's step state for the call, set by ONE launch (not one per cache)
    const size_t init_off = (ph.bytes.size() + 7) / 8 * 8, tab_bytes = init_off + n * sizeof(PackedSeqInit);
    FL_TRY(grow_packed(m, sh, (int)n, tab_bytes));
    PackedScratch &ps = sh.packed;
    float *vrows = nullptr;
    int64_t vR = 0;
    if (vf) FL_TRY(grow_verify(m, sh, any_sampled, &vrows, &vR));
    if (emb) FL_TRY(grow_embed(m, sh, T_total));
    StreamDrain drain{sh.stream};
    memcpy(ps.host_tab, ph.bytes.data(), ph.bytes.size());
    PackedSeqInit *init = reinterpret_cast<PackedSeqInit *>(ps.host_tab + init_off);
    for (size_t i = 0; i < n; i++)
        init[i] = PackedSeqInit{caches[i]->shards[0].heads_done, ids[offsets[i]], (uint32_t)pos[i], (uint32_t)caches[i]->len, 0u, sampler[i]};
    FL_HIP(hipMemcpyAsync(ps.tab, ps.host_tab, tab_bytes, hipMemcpyHostToDevice, sh.stream));
    FL_HIP(hipMemcpyAsync(sc.ids, pad ? twice : ids, (size_t)T * 4, hipMemcpyHostToDevice, sh.stream));
    const PackedTable tb = ph.at(ps.tab);
    Launcher L = make_launcher(m, sh);
    const PackedSeqInit *init_dev = reinterpret_cast<const PackedSeqInit *>((const char *)ps.tab + init_off);
    FL_TRY(launch_packed_set_states(L, tb, init_dev, (int)n, (int)(D.L * sh.Hkvs)));

    // ---- the eight-launch layer at T = T_total (+ the copy of a one-row verify pack)
    FL_TRY(launch_embed(L, dt, sh.embed, sc.ids, caches[0]->shards[0].st, sc.x_res, T, D.h));
    const int max_split = T > 1 ? ksplit_cap(T) : 1;
    const int64_t slab = T * D.h, nq = (sh.Hs + 2 * sh.Hkvs) * D.d;
    int nslab = 1;
    for (int64_t l = 0; l < D.L; l++) {
        LayerW &ly = sh.layers[l];
        const size_t kv_layer_off = (size_t)l * sh.Hkvs * D.d;
        FL_TRY(launch_rmsnorm_add(L, dt, sc.x_res, l == 0 ? nullptr : sc.delta, ly.ln1, D.eps, sc.xn, sc.inv_rms, T, D.h, nslab, slab));
        // QKV in K slabs (the bias, if any, moves into the RoPE launch, which sums the slabs anyway); no RoPE epilogue: it writes ONE cache
        int qkv_slabs = 1;
        FL_TRY(launch_linear(L, dt, ly.wqkv, sc.xn, nullptr, sc.qkv, T, nq, D.h, EPI_F32, sc.inv_rms, qkv_split(T), &qkv_slabs));
        FL_TRY(launch_rope_kv_packed(L, dt, sc.qkv, tb, sh.cos_tab, sh.sin_tab, D.max_pos, sc.q, kv_layer_off, T, sh.Hs, sh.Hkvs, D.d, qkv_slabs, ly.bqkv));
        if (any_mfma)
            FL_TRY(launch_attn_prefill_packed_mfma(L, sc.q, tb, ph.n_items, ph.TT, ph.ks, kv_layer_off, sc.ao, sh.Hs, sh.Hkvs, D.d, D.scale, D.window, attn_flops, mask));
        if (any_plain) {
            // members outside the MFMA layout (fp32 models, bf16 head shapes the MFMA kernels refuse): the single-sequence attention
            // launches on their rows of q / ao
            for (size_t i = 0; i < n; i++) {
                Cache *c = caches[i];
                if (c->v_transposed) continue;
                CacheShard &cs = c->shards[0];
                const KvLayer kv(m, c, sh, cs, l);
                const size_t roff = offsets[i] * (size_t)(sh.Hs * D.d) * es;
                const void *qi = (const char *)sc.q + roff;
                void *aoi = (char *)sc.ao + roff;
                if (counts[i] == 1) {
                    // (one token over len + 1 keys, unmasked: what both masks ask for)
                    const AttnScratch as{cs.part_m, cs.part_l, cs.part_o, cs.counters, c->nsplit, (int64_t)c->len + 1};
                    FL_TRY(attend_decode(L, m, c, sh, cs, kv, qi, aoi, as));
                } else {
                    FL_TRY(launch_attn_prefill(L, dt, qi, kv.k, kv.v, cs.st, aoi, counts[i], sh.Hs, sh.Hkvs, D.d, (int64_t)c->seq_alloc, D.scale, D.window, mask));
                }
            }
        }
        // (the copy of a one-row verify pack is not attended: it takes the row's attention output, and stays the row's exact copy in
        // every layer -- what it writes to the row's cache slot is what the row writes there)
        if (pad) FL_HIP(hipMemcpyAsync((char *)sc.ao + (size_t)(sh.Hs * D.d) * es, sc.ao, (size_t)(sh.Hs * D.d) * es, hipMemcpyDeviceToDevice, sh.stream));
        FL_TRY(launch_linear(L, dt, ly.wo, sc.ao, nullptr, sc.delta, T, D.h, sh.Hs * D.d, EPI_F32, nullptr, max_split, &nslab));
        FL_TRY(launch_rmsnorm_add(L, dt, sc.x_res, sc.delta, ly.ln2, D.eps, sc.xn, sc.inv_rms, T, D.h, nslab, slab));
        FL_TRY(launch_linear(L, dt, ly.wgu, sc.xn, nullptr, sc.act, T, 2 * sh.Ip, D.h, EPI_GATEUP, sc.inv_rms));
        FL_TRY(launch_linear(L, dt, ly.wd, sc.act, nullptr, sc.delta, T, D.h, sh.Ip, EPI_F32, nullptr, max_split, &nslab));
    }

    const int nn = (int)n;
    ScoreCall call{m, sh, score, T_total};
    if (score) {
        // ---- every row: final norm (residual + delta slabs) at T = T_total, lm_head in blocks, one score_rows launch behind each
        FL_TRY(call.begin(tg.data()));
        FL_TRY(launch_rmsnorm_add(L, dt, sc.x_res, sc.delta, sh.norm, D.eps, sc.xn, sc.inv_rms, T, D.h, nslab, slab));
        FL_TRY(lm_head_rows(m, sh, L, sc, T, call.sink(0)));
        FL_TRY(call.fetch());
    } else if (emb) {
        // ---- every row: final norm at T = T_total, which leaves the fp32 residual stream and 1/rms of every row; the pool launch
        // reads those (not the compute-dtype xn), one copy brings the vectors back
        const int64_t dims = emb->dimensions ? emb->dimensions : D.h;
        const size_t n_out = emb->pooling == FL_POOL_NONE ? T_total : n;
        FL_TRY(launch_rmsnorm_add(L, dt, sc.x_res, sc.delta, sh.norm, D.eps, sc.xn, sc.inv_rms, T, D.h, nslab, slab));
        FL_TRY(launch_pool_rows(L, sc.x_res, sc.inv_rms, sh.norm, tb.seq_off, tb.seq_cnt, (int)n_out, D.h, dims, emb->pooling, emb->normalize != 0,
                                ps.embed_part, ps.embed_out));
        FL_TRY(launch_packed_collect(L, tb, ps.result, nn));     // (the members' error words; nothing was selected)
        FL_HIP(hipMemcpyAsync(emb_out, ps.embed_out, n_out * (size_t)dims * 4, hipMemcpyDeviceToHost, sh.stream));
        FL_HIP(hipMemcpyAsync(ps.host_result, ps.result, n * 8, hipMemcpyDeviceToHost, sh.stream));
        FL_HIP(hipStreamSynchronize(sh.stream));
        for (size_t i = 0; i < n; i++)
            if (ps.host_result[2 * i + 1]) FL_FAIL(FL_ERR_HIP, "device-side wait gave up (code 0x%x) in sequence %zu", ps.host_result[2 * i + 1], i);
        for (size_t i = 0; i < n; i++) caches[i]->len += (size_t)counts[i];
        return FL_OK;
    } else if (vf) {
        // ---- every row: final norm at T = T_total, lm_head in blocks of the scoring calls' block scratch, one selection launch behind
        // each -- every row by its member's sampler (the table image's copy of it), every member's scan by whoever brings its last row
        FL_TRY(launch_rmsnorm_add(L, dt, sc.x_res, sc.delta, sh.norm, D.eps, sc.xn, sc.inv_rms, T, D.h, nslab, slab));
        VerifyPackedArgs va;
        va.rows = tb.rows; va.seq_off = tb.seq_off; va.seq_cnt = tb.seq_cnt;
        va.ss = &init_dev->ss; va.ss_stride = sizeof(PackedSeqInit);
        va.ids = sc.ids; va.out = ps.verify_out;
        const size_t V = (size_t)D.V;
        // fp32: a block never exceeds the 64 rows of the fp32 row-stream GEMM, and no block but a whole pack's is one row (below), so
        // that blocks of 3 .. 64 rows and more all run lm_head through that one kernel and what a row selects does not depend on the
        // score_rows switch (beyond 64 rows the planner takes the MFMA kernel, at one row the GEMV: other sums in the last bits).
        // bf16: the planner picks lm_head's kernel by the block's rows, so two switch values agree bit for bit only where it picks
        // the same one.
        const int64_t block = dt == FL_DTYPE_F32 ? std::min<int64_t>(vR, 64) : vR;
        TicketReset tickets{ps.verify_out, sh.stream};
        AllRows rows{vrows, block, [&](Launcher &L2, int64_t r0, int64_t nb) -> int {
            nb = std::min<int64_t>(nb, (int64_t)T_total - r0);           // (the copy of a one-row pack is neither selected nor returned)
            if (nb <= 0) return FL_OK;
            FL_TRY(launch_verify_packed(L2, vrows, D.V, (int)r0, (int)nb, (int)T_total, va, ps.verify_prob, any_sampled));
            // (the diagnostic copy: stream-ordered, so the next block's lm_head overwrites the rows only behind it)
            if (logits_out) FL_HIP(hipMemcpyAsync(logits_out + (size_t)r0 * V, vrows, (size_t)nb * V * 4, hipMemcpyDeviceToHost, sh.stream));
            return FL_OK;
        }};
        rows.no_one_row_tail = true;
        FL_TRY(lm_head_rows(m, sh, L, sc, T, rows));
        // ... the members' error words into the same block: ids, accepted counts and error words come back in one copy
        FL_TRY(launch_packed_collect(L, tb, ps.verify_out + kVerifyPackedAux, nn));
        FL_HIP(hipMemcpyAsync(ps.host_verify, ps.verify_out, (size_t)kVerifyPackedWords * 4, hipMemcpyDeviceToHost, sh.stream));
        FL_HIP(hipStreamSynchronize(sh.stream));
        const uint32_t *hv = ps.host_verify;
        for (size_t i = 0; i < n; i++) {
            if (hv[kVerifyPackedTicket + i]) FL_FAIL(FL_ERR_HIP, "packed verify step: the ticket of sequence %zu came back as %u, not 0", i, hv[kVerifyPackedTicket + i]);
            if (hv[kVerifyPackedAux + 2 * i + 1]) FL_FAIL(FL_ERR_HIP, "device-side wait gave up (code 0x%x) in sequence %zu", hv[kVerifyPackedAux + 2 * i + 1], i);
            if (hv[kVerifyPackedNacc + i] >= (uint32_t)counts[i]) FL_FAIL(FL_ERR_HIP, "packed verify step: accepted count %u of sequence %zu out of range", hv[kVerifyPackedNacc + i], i);
        }
        for (size_t i = 0; i < n; i++) {
            const size_t got = (size_t)hv[kVerifyPackedNacc + i] + 1;
            for (size_t k = 0; k < got; k++) vf->tokens_out[offsets[i] + k] = hv[offsets[i] + k];
            vf->n_out[i] = got;
            caches[i]->len += got;                               // rejected rows' K/V stay behind the length; the next append overwrites them
        }
        tickets.armed = false;
        return FL_OK;
    } else {
        // ---- the n last rows: gather, final norm (residual + delta slabs), lm_head once at T = n, token selection per sequence
        const int64_t lslab = (int64_t)nn * D.h;
        FL_TRY(launch_gather_last_rows(L, sc.x_res, tb, ps.xl, nn, D.h, 1, 0, 0));
        FL_TRY(launch_gather_last_rows(L, sc.delta, tb, ps.dl, nn, D.h, nslab, slab, lslab));
        FL_TRY(launch_rmsnorm_add(L, dt, ps.xl, ps.dl, sh.norm, D.eps, ps.xnl, ps.inv_rms, nn, D.h, nslab, lslab));
        FL_TRY(launch_linear(L, dt, sh.lm_head, ps.xnl, nullptr, ps.logits, nn, D.V, D.h, EPI_F32, ps.inv_rms));
        FL_TRY(launch_select_advance_batch(L, ps.logits, D.V, tb.seqs, nn, 0));
    }

    // ---- back to the host (tokens and error words gathered for one copy); only when every member's step state is clean do the caches grow
    FL_TRY(launch_packed_collect(L, tb, ps.result, nn));
    if (logits_out) FL_HIP(hipMemcpyAsync(logits_out, ps.logits, n * (size_t)D.V * 4, hipMemcpyDeviceToHost, sh.stream));
    FL_HIP(hipMemcpyAsync(ps.host_result, ps.result, n * 8, hipMemcpyDeviceToHost, sh.stream));
    FL_HIP(hipStreamSynchronize(sh.stream));
    for (size_t i = 0; i < n; i++)
        if (ps.host_result[2 * i + 1]) FL_FAIL(FL_ERR_HIP, "device-side wait gave up (code 0x%x) in sequence %zu", ps.host_result[2 * i + 1], i);
    for (size_t i = 0; i < n; i++) {
        caches[i]->len += (size_t)counts[i];
        if (tokens_out) tokens_out[i] = ps.host_result[2 * i];
    }
    if (score) call.end();
    return FL_OK;
}

}  // namespace

int batch_prefill(Model *m, Cache *const *caches, size_t n, const uint32_t *ids, const size_t *offsets, const size_t *pos,
                  const fl_sampler *samplers, uint32_t *tokens_out, float *logits_out) {
    return packed_forward(m, caches, n, ids, offsets, pos, samplers, tokens_out, logits_out, nullptr);
}

int check_embed(const fl_embed *e, int64_t h) {
    if (!e) FL_FAIL(FL_ERR_BAD_ARGUMENT, "null fl_embed (opts)");
    if (e->struct_size != sizeof(fl_embed)) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_embed.struct_size is %u, expected %zu", e->struct_size, sizeof(fl_embed));
    if (e->pooling < FL_POOL_LAST || e->pooling > FL_POOL_NONE) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_embed.pooling %d is not an fl_pooling", e->pooling);
    if (e->mask != FL_MASK_CAUSAL && e->mask != FL_MASK_FULL) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_embed.mask %d is not an fl_attn_mask", e->mask);
    if (e->normalize != 0 && e->normalize != 1) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_embed.normalize is %d, not 0 or 1", e->normalize);
    if (e->dimensions < 0) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_embed.dimensions %lld is negative", (long long)e->dimensions);
    if (e->_reserved[0] || e->_reserved[1]) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_embed._reserved must be 0");
    if (h > 0 && e->dimensions > h) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_embed.dimensions %lld exceeds the hidden size %lld", (long long)e->dimensions, (long long)h);
    return FL_OK;
}

int batch_embed(Model *m, Cache *const *caches, size_t n, const uint32_t *ids, const size_t *offsets, const size_t *pos, const fl_embed *opts,
                float *out) {
    FL_TRY(check_embed(opts, 0));               // the struct's own errors first: they need neither model nor device
    if (!out) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_batch_embed: null out");
    return packed_forward(m, caches, n, ids, offsets, pos, nullptr, nullptr, nullptr, nullptr, nullptr, opts, out);
}

int batch_score(Model *m, Cache *const *caches, size_t n, const uint32_t *ids, const size_t *offsets, const size_t *pos, const fl_score *sc) {
    FL_TRY(check_score(sc, 0, 0));              // the struct's own errors first: they need neither model nor device
    return packed_forward(m, caches, n, ids, offsets, pos, nullptr, nullptr, nullptr, sc);
}

int batch_verify(Model *m, Cache *const *caches, size_t n, const uint32_t *ids, const size_t *offsets, const size_t *pos,
                 const fl_sampler *samplers, uint32_t *tokens_out, size_t *n_out, float *logits_out) {
    // everything that needs neither the model nor a cache, before either is looked at
    if (n < 1 || n > (size_t)kMaxBatch) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_batch_verify: %zu sequences: a packed verify takes 1..%d", n, kMaxBatch);
    if (n_out) for (size_t i = 0; i < n; i++) n_out[i] = 0;
    if (!caches || !ids || !offsets || !pos) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_batch_verify: null caches, ids, offsets or pos");
    if (!tokens_out || !n_out) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_batch_verify: null tokens_out or n_out");
    SampleState probe;
    if (samplers) for (size_t i = 0; i < n; i++) FL_TRY(make_sampler(samplers + i, 0, &probe));
    FL_TRY(check_pack_shape(kWordsVerify, caches, n, offsets, (size_t)FL_VERIFY_MAX_DRAFT + 1));   // (packed_forward's own, here ahead of the model)
    if (!m) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_batch_verify: null model");
    const VerifyMode vf{tokens_out, n_out};
    return packed_forward(m, caches, n, ids, offsets, pos, samplers, nullptr, logits_out, nullptr, &vf);
}

int batch_decode_lookup(Model *m, Cache *const *caches, size_t n, const uint32_t *corpus, const size_t *corpus_offsets, const uint32_t *first,
                        const size_t *pos, const size_t *n_steps, const int64_t *eos, const fl_lookup *opts, const fl_sampler *samplers,
                        uint32_t *tokens_out, size_t *n_out, fl_spec_stats *stats) {
    if (n < 1 || n > (size_t)kMaxBatch) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_batch_decode_lookup: n = %zu sequences, a packed verify takes 1..%d", n, kMaxBatch);
    if (n_out) for (size_t i = 0; i < n; i++) n_out[i] = 0;
    if (stats) for (size_t i = 0; i < n; i++) stats[i] = fl_spec_stats{};
    FL_TRY(check_lookup(opts));
    SampleState probe;
    if (samplers) for (size_t i = 0; i < n; i++) FL_TRY(make_sampler(samplers + i, 0, &probe));   // their argument errors, before the handles are looked at
    if (!n_out) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_batch_decode_lookup: null n_out");
    if (!caches || !corpus_offsets || !first || !pos || !n_steps)
        FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_batch_decode_lookup: null caches, corpus_offsets, first_tokens, pos or n_steps");
    for (size_t i = 0; i < n; i++)
        if (corpus_offsets[i + 1] < corpus_offsets[i]) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_batch_decode_lookup: corpus_offsets decrease at sequence %zu", i);
    if (corpus_offsets[n] > corpus_offsets[0] && !corpus) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_batch_decode_lookup: null corpus");
    size_t stride = 0;
    for (size_t i = 0; i < n; i++) stride = std::max(stride, n_steps[i]);
    if (stride == 0) return FL_OK;
    if (!tokens_out) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_batch_decode_lookup: null tokens_out");
    if (!m) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_batch_decode_lookup: null model or cache");
    for (size_t i = 0; i < n; i++) {
        if (!caches[i] || caches[i]->m != m) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_batch_decode_lookup: cache %zu is null or belongs to another model", i);
        for (size_t j = 0; j < i; j++) if (caches[j] == caches[i]) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_batch_decode_lookup: cache %zu appears twice in the call", i);
        FL_TRY(refuse_logit_rules(caches[i], "fl_batch_decode_lookup"));
        FL_TRY(refuse_guide(caches[i], "fl_batch_decode_lookup"));
        if (n_steps[i] == 0) continue;
        FL_TRY(check_call(m, caches[i], n_steps[i], pos[i]));
        FL_TRY(check_token(m, first[i], "token"));
    }
    if (m->tp > 1 || m->shards.size() != 1) FL_FAIL(FL_ERR_UNSUPPORTED, "a packed verify runs on one GPU (tp_size %d)", m->tp);
    const size_t V = (size_t)m->D.V;
    struct Member { std::vector<uint32_t> hist; uint32_t tok; size_t emitted, L0; bool done; };
    std::vector<Member> mem(n);
    for (size_t i = 0; i < n; i++) {
        Member &b = mem[i];
        b.hist.reserve(corpus_offsets[i + 1] - corpus_offsets[i] + 1 + n_steps[i] + FL_VERIFY_MAX_DRAFT + 1);
        for (size_t k = corpus_offsets[i]; k < corpus_offsets[i + 1]; k++) b.hist.push_back(corpus[k]);
        b.hist.push_back(first[i]);
        b.tok = first[i]; b.emitted = 0; b.L0 = caches[i]->len; b.done = n_steps[i] == 0;
    }
    std::vector<Cache *> pc;
    std::vector<size_t> who, poff, ppos, pn(n);
    std::vector<uint32_t> pids, got;
    std::vector<fl_sampler> psp;
    for (;;) {
        pc.clear(); who.clear(); pids.clear(); ppos.clear(); psp.clear();
        poff.assign(1, 0);
        for (size_t i = 0; i < n; i++) {
            Member &b = mem[i];
            if (b.done) continue;
            Cache *c = caches[i];
            // room: this step caches `tok` and up to n_draft drafts, and every later token still needs its own position
            size_t limit = n_steps[i] - b.emitted - 1;
            limit = std::min(limit, c->max_seq - c->len - 1);
            limit = std::min(limit, (size_t)m->D.max_pos - (pos[i] + b.emitted) - 1);
            if (m->D.window >= 0) limit = std::min(limit, (size_t)m->D.window);
            uint32_t draft[FL_VERIFY_MAX_DRAFT + 1];
            size_t nd = lookup_draft(b.hist.data(), b.hist.size(), opts->max_draft, opts->ngram_max, opts->ngram_min, limit, draft);
            for (size_t k = 0; k < nd; k++) if (draft[k] >= V) { nd = k; break; }      // (a corpus id the model does not have ends the draft)
            who.push_back(i); pc.push_back(c);
            pids.push_back(b.tok);
            for (size_t k = 0; k < nd; k++) pids.push_back(draft[k]);
            poff.push_back(pids.size());
            ppos.push_back(pos[i] + b.emitted);
            // token k of the request is drawn with word k: this step's row r with word draws_done + emitted + r, whatever was rejected before
            if (samplers) { fl_sampler sp = samplers[i]; sp.draws_done += b.emitted; psp.push_back(sp); }
        }
        if (who.empty()) break;
        got.resize(pids.size());
        FL_TRY(batch_verify(m, pc.data(), who.size(), pids.data(), poff.data(), ppos.data(), samplers ? psp.data() : nullptr, got.data(), pn.data(), nullptr));
        for (size_t a = 0; a < who.size(); a++) {
            const size_t i = who[a];
            Member &b = mem[i];
            const size_t nd = poff[a + 1] - poff[a] - 1, cnt = pn[a];
            if (stats) { stats[i].steps += 1; stats[i].drafted += nd; stats[i].accepted += cnt - 1; }
            for (size_t k = 0; k < cnt && !b.done; k++) {
                const uint32_t t = got[poff[a] + k];
                if (eos && eos[i] >= 0 && (int64_t)t == eos[i]) {
                    // the forward that produced EOS was needed; what was accepted after it is dropped (fl_decode_greedy's length)
                    caches[i]->len = b.L0 + b.emitted + 1;
                    b.done = true;
                    break;
                }
                tokens_out[i * stride + b.emitted++] = t;
                b.hist.push_back(t);
                b.tok = t;
            }
            n_out[i] = b.emitted;
            if (b.emitted >= n_steps[i]) b.done = true;
        }
    }
    return FL_OK;
}

}  // namespace fl
