// prefill_packed.hip -- fl_batch_prefill: several prompts of one model in ONE forward (model.h: batch_prefill).
// Up to about 128 rows the projections of a prompt are a weight stream, so n short prompts forwarded one after the other read the
// weights n times; packed, their tokens are the rows of one forward.  Everything row-wise runs at T = the total token count through
// the same launches (and the same planner) as a single prompt; RoPE / KV append and attention go through k_prefill_packed.hip, which
// finds every row's own cache in a device table; the final norm, lm_head and token selection run on the n last rows only.
// Eager launches: no graph, no residual or RoPE epilogues in the projections.
#include "model.h"

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

struct StreamDrain {            // an early return leaves nothing in flight that reads the call's host buffers
    hipStream_t s;
    ~StreamDrain() { (void)hipStreamSynchronize(s); }
};

// batch_prefill, or -- score != null -- batch_score: the same checks and the same layers; behind them either the n last rows go through
// the final norm, lm_head and token selection, or ALL rows go through the final norm and lm_head in blocks, each scored (model.h: ScoreCall)
int packed_forward(Model *m, Cache *const *caches, size_t n, const uint32_t *ids, const size_t *offsets, const size_t *pos,
                   const fl_sampler *samplers, uint32_t *tokens_out, float *logits_out, const fl_score *score) {
    // ---- everything that can be refused is refused here, before the device or any cache is touched
    if (!m || !caches || !ids || !offsets || !pos) FL_FAIL(FL_ERR_BAD_ARGUMENT, "null argument");
    if (n < 1 || n > (size_t)kMaxBatch) FL_FAIL(FL_ERR_BAD_ARGUMENT, "%zu sequences: a packed prefill takes 1..%d", n, kMaxBatch);
    if (m->tp > 1 || m->shards.size() != 1) FL_FAIL(FL_ERR_UNSUPPORTED, "a packed prefill runs on one GPU (tp_size %d)", m->tp);
    if (offsets[0] != 0) FL_FAIL(FL_ERR_BAD_ARGUMENT, "offsets[0] is %zu, not 0", offsets[0]);
    for (size_t i = 0; i < n; i++) {
        if (offsets[i + 1] <= offsets[i]) FL_FAIL(FL_ERR_BAD_ARGUMENT, "sequence %zu is empty (offsets must increase)", i);
        if (!caches[i] || caches[i]->m != m) FL_FAIL(FL_ERR_BAD_ARGUMENT, "cache %zu is null or belongs to another model", i);
        for (size_t j = 0; j < i; j++) if (caches[j] == caches[i]) FL_FAIL(FL_ERR_BAD_ARGUMENT, "cache %zu appears twice in the call", i);
        if (tokens_out) FL_TRY(refuse_logit_rules(caches[i], "fl_batch_prefill with tokens_out"));   // (its selection reads the raw rows)
        if (tokens_out) FL_TRY(refuse_guide(caches[i], "fl_batch_prefill with tokens_out"));
    }
    const size_t T_total = offsets[n];
    for (size_t r = 0; r < T_total; r++) FL_TRY(check_token(m, ids[r], "token"));
    const size_t chunk_max = (size_t)tune(TK_PREFILL_CHUNK);
    if (T_total > chunk_max) FL_FAIL(FL_ERR_UNSUPPORTED, "%zu tokens in one packed prefill: at most %zu (FL_PREFILL_CHUNK); split the call", T_total, chunk_max);
    for (size_t i = 0; i < n; i++) FL_TRY(check_call(m, caches[i], offsets[i + 1] - offsets[i], pos[i]));
    std::vector<SampleState> sampler(n);
    for (size_t i = 0; i < n; i++) FL_TRY(make_sampler(samplers ? samplers + i : nullptr, m->D.V, &sampler[i]));
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
    const int64_t T = (int64_t)T_total;
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
    packed_table_build(refs.data(), counts.data(), vt.data(), (int)n, sh.Hs, sh.Hkvs, D.d, &ph);
    // ... and behind it every member's step state for the call, set by ONE launch (not one per cache)
    const size_t init_off = (ph.bytes.size() + 7) / 8 * 8, tab_bytes = init_off + n * sizeof(PackedSeqInit);
    FL_TRY(grow_packed(m, sh, (int)n, tab_bytes));
    PackedScratch &ps = sh.packed;
    StreamDrain drain{sh.stream};
    memcpy(ps.host_tab, ph.bytes.data(), ph.bytes.size());
    PackedSeqInit *init = reinterpret_cast<PackedSeqInit *>(ps.host_tab + init_off);
    for (size_t i = 0; i < n; i++)
        init[i] = PackedSeqInit{caches[i]->shards[0].heads_done, ids[offsets[i]], (uint32_t)pos[i], (uint32_t)caches[i]->len, 0u, sampler[i]};
    FL_HIP(hipMemcpyAsync(ps.tab, ps.host_tab, tab_bytes, hipMemcpyHostToDevice, sh.stream));
    FL_HIP(hipMemcpyAsync(sc.ids, ids, T_total * 4, hipMemcpyHostToDevice, sh.stream));
    const PackedTable tb = ph.at(ps.tab);
    Launcher L = make_launcher(m, sh);
    FL_TRY(launch_packed_set_states(L, tb, reinterpret_cast<const PackedSeqInit *>((const char *)ps.tab + init_off), (int)n, (int)(D.L * sh.Hkvs)));

    // ---- the eight-launch layer at T = T_total
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
            FL_TRY(launch_attn_prefill_packed_mfma(L, sc.q, tb, ph.n_items, ph.TT, ph.ks, kv_layer_off, sc.ao, sh.Hs, sh.Hkvs, D.d, D.scale, D.window, attn_flops));
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
                    const AttnScratch as{cs.part_m, cs.part_l, cs.part_o, cs.counters, c->nsplit, (int64_t)c->len + 1};
                    FL_TRY(attend_decode(L, m, c, sh, cs, kv, qi, aoi, as));
                } else {
                    FL_TRY(launch_attn_prefill(L, dt, qi, kv.k, kv.v, cs.st, aoi, counts[i], sh.Hs, sh.Hkvs, D.d, (int64_t)c->seq_alloc, D.scale, D.window));
                }
            }
        }
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

int batch_score(Model *m, Cache *const *caches, size_t n, const uint32_t *ids, const size_t *offsets, const size_t *pos, const fl_score *sc) {
    FL_TRY(check_score(sc, 0, 0));              // the struct's own errors first: they need neither model nor device
    return packed_forward(m, caches, n, ids, offsets, pos, nullptr, nullptr, nullptr, sc);
}

}  // namespace fl
