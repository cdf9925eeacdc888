// batch.hip -- batched decode: a fixed set of caches of one model stepped together (model.h: Batch).
#include "model.h"

#include <algorithm>
#include <memory>

namespace fl {

// ------------------------------------------------------------------------------- batched decode (row N4)
Batch::~Batch() {
    if (!m) return;
    std::lock_guard<std::mutex> lock(m->mu);
    Shard &sh = m->shards[0];
    (void)hipSetDevice(sh.device);
    (void)hipStreamSynchronize(sh.stream);
    for (auto g : graph) if (g) (void)hipGraphExecDestroy(g);
    for (void *p : allocs) (void)hipFree(p);
    if (host_lp) (void)hipHostFree(host_lp);
    if (host_tokens) (void)hipHostFree(host_tokens);
    if (host_states) (void)hipHostFree(host_states);
}

int batch_create(Model *m, Cache *const *caches, size_t B, Batch **out) {
    if (!m || !caches || !out) FL_FAIL(FL_ERR_BAD_ARGUMENT, "null argument");
    if (B < 1 || B > (size_t)kMaxBatch) FL_FAIL(FL_ERR_BAD_ARGUMENT, "batch size %zu not in 1..%d", B, kMaxBatch);
    // one GPU, or -- round 5 -- one rank of a multi-process tensor-parallel group (every rank builds the same batch and calls the same
    // entry points: the step's all-reduces and logits gather are collectives)
    const bool tp_rank = m->tp > 1 && m->tp_mode == FL_TP_MULTI_PROCESS && m->shards.size() == 1;
    if (m->shards.size() != 1 || (m->tp != 1 && !tp_rank)) FL_FAIL(FL_ERR_UNSUPPORTED, "batched decode runs on one GPU or on the ranks of an FL_TP_MULTI_PROCESS group");
    if (tp_rank && (!m->shards[0].pc.connected || !m->vocab_parallel || m->shards[0].Vs % 4))
        FL_FAIL(FL_ERR_UNSUPPORTED, "batched decode on a tensor-parallel group needs connected peer inboxes and a vocabulary shard that is a multiple of 4");
    const Dims &D = m->D;
    Shard &sh = m->shards[0];
    // fp32 models (the literal-parity mode) and caches without the MFMA attention layout: the weights are still read once per step for
    // all B rows; embedding, RoPE / KV append and attention run as the single-sequence kernels on row i of the batch (3 B small launches
    // per layer, replayed from the step's graph)
    bool per_seq = m->dtype != FL_DTYPE_BF16;
    for (size_t i = 0; i < B; i++) {
        if (!caches[i] || caches[i]->m != m) FL_FAIL(FL_ERR_BAD_ARGUMENT, "cache %zu is null or belongs to another model", i);
        if (!caches[i]->v_transposed) per_seq = true;
        for (size_t j = 0; j < i; j++) if (caches[j] == caches[i]) FL_FAIL(FL_ERR_BAD_ARGUMENT, "cache %zu appears twice in the batch", i);
    }
    if (per_seq && tp_rank) FL_FAIL(FL_ERR_UNSUPPORTED, "batched decode on a tensor-parallel group is bf16 with the MFMA attention layout (head_dim 64/128, group <= 8)");
    std::unique_ptr<Batch> b(new Batch());
    std::lock_guard<std::mutex> lock(m->mu);
    b->m = m; b->B = (int)B; b->per_seq = per_seq;
    if (per_seq && attn_decode_batch_supported(D.d)) {
        b->plain = true;
        for (size_t i = 0; i < B; i++) if (caches[i]->v_transposed) b->plain = false;
    }
    b->caches.assign(caches, caches + B);
    // B >= 3: the prefill-shaped step (separate norm / RoPE launches) with the wide projections on the LDS-DMA ring kernel
    b->dma = !per_seq && B >= (size_t)tune(TK_BATCH_DMA_MIN) && gemv_dma_supported((int)B, 2 * sh.Ip, D.h, EPI_GATEUP, 0) &&
             gemv_dma_supported((int)B, sh.Vs, D.h, EPI_F32, 0) && gemv_dma_ksplit(D.h, 0, EPI_GATEUP) == 1;
    const bool gemv_rows = B <= (size_t)kMaxBatchGemv && !tp_rank && !per_seq;   // the streaming GEMV forms hold at most eight rows (and know no all-reduce)
    if (gemv_rows) {
        b->nks_o = gemv_batch_ksplit((int)B, sh.Hs * D.d, D.h, EPI_F32);
        b->nks_down = gemv_batch_ksplit((int)B, sh.Ip, D.h, EPI_F32);
        if (gemv_batch_ksplit((int)B, D.h, 2 * sh.Ip, EPI_GATEUP) != 1) FL_FAIL(FL_ERR_UNSUPPORTED, "hidden size %lld too large for the batched norm prologue", (long long)D.h);
    }
    FL_HIP(hipSetDevice(sh.device));
    std::vector<SeqRef> refs(B);
    for (size_t i = 0; i < B; i++) {
        CacheShard &cs = caches[i]->shards[0];
        refs[i] = SeqRef{cs.st, cs.ss, cs.k, cs.v, cs.part_m, cs.part_l, cs.part_o, cs.counters, cs.out_tokens, cs.sel_scratch,
                         (int)caches[i]->seq_alloc, caches[i]->nsplit};
        b->max_nsplit = std::max(b->max_nsplit, caches[i]->nsplit);
    }
    const size_t es = m->esize();
    const int nsl = std::max(b->nks_o, b->nks_down);
    FL_TRY(dev_alloc(b->allocs, (void **)&b->seqs_dev, sizeof(SeqRef) * B, nullptr));
    FL_TRY(dev_alloc(b->allocs, (void **)&b->x_res, B * D.h * 4, nullptr));
    FL_TRY(dev_alloc(b->allocs, (void **)&b->x_res2, B * D.h * 4, nullptr));
    FL_TRY(dev_alloc(b->allocs, (void **)&b->delta, (size_t)nsl * B * D.h * 4, nullptr));
    FL_TRY(dev_alloc(b->allocs, &b->q, B * sh.Hs * D.d * es, nullptr));
    FL_TRY(dev_alloc(b->allocs, &b->ao, B * sh.Hs * D.d * es, nullptr));
    FL_TRY(dev_alloc(b->allocs, &b->act, B * sh.Ip * es, nullptr));
    FL_TRY(dev_alloc(b->allocs, (void **)&b->logits, B * D.V * 4, nullptr));
    if (tp_rank) {
        FL_TRY(dev_alloc(b->allocs, (void **)&b->logits_local, B * sh.Vs * 4, nullptr));
        FL_TRY(dev_alloc(b->allocs, (void **)&b->logits_ranks, B * D.V * 4, nullptr));
    }
    // B >= 7: every projection through the short-prompt GEMM with the norm and RoPE / KV append as their own small
    // launches, i.e. the prefill pipeline at T = B with per-sequence positions and caches.  Measured (Mistral-7B,
    // ms per step, unfused vs fused): B = 3 4.16 / 3.87, 4 4.21 / 3.99, 6 4.24 / 4.18, 8 4.26 / 4.38
    b->unfused = B >= (size_t)(tune(TK_BATCH_UNFUSED_MIN) >= 0 ? tune(TK_BATCH_UNFUSED_MIN) : (b->dma ? 3 : 7)) && gemm_skinny_supported((int64_t)B, D.h, D.h) &&
                 gemm_skinny_supported((int64_t)B, D.h, sh.Ip);
    // more than eight streams, or a tensor-parallel rank: always the prefill-shaped step (launch_linear finds a kernel for every shape)
    if (!gemv_rows) b->unfused = true;
    if (b->unfused) {
        FL_TRY(alloc_scratch(m, sh, b->sc, (int64_t)B, &b->allocs));
    }
    FL_HIP(hipMemcpyAsync(b->seqs_dev, refs.data(), sizeof(SeqRef) * B, hipMemcpyHostToDevice, sh.stream));
    FL_HIP(hipStreamSynchronize(sh.stream));                  // refs is a stack vector
    FL_HIP(hipHostMalloc((void **)&b->host_tokens, B * kBatchChunk * 4, hipHostMallocDefault));
    FL_HIP(hipHostMalloc((void **)&b->host_states, B * sizeof(StepState), hipHostMallocDefault));
    m->refs.fetch_add(1);
    *out = b.release();
    return FL_OK;
}

// Continuous batching: sequence `slot` of a batch leaves (EOS, cancelled) and another stream's cache takes its place,
// without rebuilding the batch.  Every kernel of the step reads a sequence's pointers, length and split count from its SeqRef in
// device memory, so the step's captured graph stays valid: the swap is one 80-byte copy.  The graph is dropped (and re-captured by
// the next step) only where launch geometry or node arguments depend on the caches: a larger attention split count than any
// sequence had so far, or the per-sequence launches of a mixed-layout batch.
int batch_replace(Batch *b, size_t slot, Cache *c) {
    if (!b || !c) FL_FAIL(FL_ERR_BAD_ARGUMENT, "null argument");
    Model *m = b->m;
    if (slot >= (size_t)b->B) FL_FAIL(FL_ERR_BAD_ARGUMENT, "slot %zu not in 0..%d", slot, b->B - 1);
    if (c->m != m) FL_FAIL(FL_ERR_BAD_ARGUMENT, "the cache belongs to another model");
    for (int i = 0; i < b->B; i++)
        if (b->caches[i] == c && (size_t)i != slot) FL_FAIL(FL_ERR_BAD_ARGUMENT, "the cache is sequence %d of this batch already", i);
    if (b->caches[slot] == c) return FL_OK;
    if (!b->per_seq && !c->v_transposed) FL_FAIL(FL_ERR_UNSUPPORTED, "this batch runs the MFMA batch attention: the new cache must be in that layout too");
    if (b->plain && c->v_transposed) FL_FAIL(FL_ERR_UNSUPPORTED, "this batch runs the plain-layout batch attention: the new cache must be in that layout too");
    std::lock_guard<std::mutex> lock(m->mu);
    Shard &sh = m->shards[0];
    FL_HIP(hipSetDevice(sh.device));
    FL_HIP(hipStreamSynchronize(sh.stream));
    CacheShard &cs = c->shards[0];
    const SeqRef ref{cs.st, cs.ss, cs.k, cs.v, cs.part_m, cs.part_l, cs.part_o, cs.counters, cs.out_tokens, cs.sel_scratch, (int)c->seq_alloc, c->nsplit};
    FL_HIP(hipMemcpy(b->seqs_dev + slot, &ref, sizeof(SeqRef), hipMemcpyHostToDevice));
    b->caches[slot] = c;
    const bool regraph = c->nsplit > b->max_nsplit || (b->per_seq && !b->plain);
    b->max_nsplit = std::max(b->max_nsplit, c->nsplit);
    for (auto &g : b->graph) if (regraph && g) { (void)hipGraphExecDestroy(g); g = nullptr; }
    if (b->rule_ctls) {                                           // the rules launch finds the new member's control block (null: none)
        LogitRulesCtl *ctl = c->rules_on ? cs.rule_ctl : nullptr;
        FL_HIP(hipMemcpy(b->rule_ctls + slot, &ctl, sizeof ctl, hipMemcpyHostToDevice));
    }
    if (b->guide_ctls) {                                          // ... and the guide launch
        GuideCtl *ctl = c->guide ? cs.guide_ctl : nullptr;
        FL_HIP(hipMemcpy(b->guide_ctls + slot, &ctl, sizeof ctl, hipMemcpyHostToDevice));
    }
    return FL_OK;
}

static int enqueue_batch_step_unfused(Batch *b, int kind);

// Token selection of every sequence.  kStepRules: a member has logit rules -- one launch first leaves every row adjusted by its own
// member's rules (copied through for a member without) in logits_adj; kStepGuide: a member has a guide -- one launch then leaves every
// row (adjusted or raw) masked under its own member's state (copied through for a member without) in logits_guided; the selection
// reads the last of them.  Neither: the launch there always was
static int batch_select(Batch *b, Launcher &L, int kind) {
    const int64_t V = b->m->D.V;
    const float *rows = b->logits;
    if (kind & kStepRules) {
        LogitRulesSrc src;
        src.seqs = b->seqs_dev; src.ctls = b->rule_ctls; src.out = b->logits_adj;
        FL_TRY(launch_logit_rules(L, rows, V, b->B, src));
        rows = b->logits_adj;
    }
    if (kind & kStepGuide) {
        GuideSrc src;
        src.seqs = b->seqs_dev; src.ctls = b->guide_ctls; src.out = b->logits_guided;
        FL_TRY(launch_guide_mask(L, rows, V, b->B, src));
        rows = b->logits_guided;
    }
    return launch_select_advance_batch(L, rows, V, b->seqs_dev, b->B, 1);
}

// One decode step of the whole batch: the 5-launch layer of enqueue_decode_fused with B activation rows.
static int enqueue_batch_step(Batch *b, int kind = 0) {
    if (b->unfused) return enqueue_batch_step_unfused(b, kind);
    Model *m = b->m;
    const Dims &D = m->D;
    Shard &sh = m->shards[0];
    Launcher L = make_launcher(m, sh);
    const int B = b->B;
    const long long slab = (long long)B * D.h;
    for (int64_t l = 0; l < D.L; l++) {
        LayerW &ly = sh.layers[l];
        GemvBatchArgs a;
        a.B = B; a.seqs = b->seqs_dev;
        a.W = ly.wqkv; a.bias = ly.bqkv; a.N = (int)((sh.Hs + 2 * sh.Hkvs) * D.d); a.K = (int)D.h; a.nks = 1;
        a.epi = EPI_QKV_ROPE; a.pro = PRO_NORM; a.norm_w = ly.ln1; a.eps = D.eps;
        if (l == 0) { a.embed = sh.embed; a.x_out = b->x_res2; }
        else { a.x_in = b->x_res; a.delta = b->delta; a.n_slab = b->nks_down; a.slab_stride = slab; a.x_out = b->x_res2; }
        a.cos_tab = sh.cos_tab; a.sin_tab = sh.sin_tab; a.q_out = b->q; a.kv_layer_off = (size_t)l * sh.Hkvs * D.d;
        a.H = (int)sh.Hs; a.Hkv = (int)sh.Hkvs; a.d = (int)D.d; a.max_pos = (int)D.max_pos;
        FL_TRY(launch_gemv_batch(L, a));
        FL_TRY(launch_attn_decode_mfma_batch(L, b->q, b->seqs_dev, B, b->max_nsplit, (size_t)l * sh.Hkvs * D.d, b->ao, sh.Hs, sh.Hkvs,
                                             D.d, D.scale, 0.0));
        GemvBatchArgs o;
        o.B = B; o.W = ly.wo; o.x = b->ao; o.out = b->delta; o.N = (int)D.h; o.K = (int)(sh.Hs * D.d); o.nks = b->nks_o;
        FL_TRY(launch_gemv_batch(L, o));
        GemvBatchArgs g;
        g.B = B; g.seqs = b->seqs_dev; g.W = ly.wgu; g.out = b->act; g.N = (int)(2 * sh.Ip); g.K = (int)D.h; g.epi = EPI_GATEUP; g.pro = PRO_NORM;
        g.x_in = b->x_res2; g.delta = b->delta; g.n_slab = b->nks_o; g.slab_stride = slab; g.norm_w = ly.ln2; g.eps = D.eps; g.x_out = b->x_res;
        FL_TRY(launch_gemv_batch(L, g));
        GemvBatchArgs d;
        d.B = B; d.W = ly.wd; d.x = b->act; d.out = b->delta; d.N = (int)D.h; d.K = (int)sh.Ip; d.nks = b->nks_down;
        FL_TRY(launch_gemv_batch(L, d));
    }
    GemvBatchArgs h;
    h.B = B; h.seqs = b->seqs_dev; h.W = sh.lm_head; h.out = b->logits; h.N = (int)D.V; h.K = (int)D.h; h.pro = PRO_NORM;
    h.x_in = b->x_res; h.delta = b->delta; h.n_slab = b->nks_down; h.slab_stride = slab; h.norm_w = sh.norm; h.eps = D.eps;
    FL_TRY(launch_gemv_batch(L, h));
    return batch_select(b, L, kind);
}

// The same step as 8 launches per layer: rmsnorm_add -> QKV GEMM -> RoPE / KV append -> attention -> o_proj GEMM (K
// slabs) -> rmsnorm_add (sums them) -> gate/up GEMM -> down GEMM (K slabs); launch_linear picks gemm_skinny_kernel.
static int enqueue_batch_step_unfused(Batch *b, int kind) {
    Model *m = b->m;
    const Dims &D = m->D;
    Shard &sh = m->shards[0];
    Scratch &sc = b->sc;
    Launcher L = make_launcher(m, sh);
    const int dt = m->dtype, B = b->B;
    const int64_t T = B, slab = T * D.h;
    int nslab = 1;
    // the two wide projections (gate/up, lm_head: thousands of 16-row units) stream fastest through the LDS-DMA ring kernel;
    // the narrow ones (QKV, o_proj, down_proj: one or two units per CU) through K slices of the short-prompt GEMM
    auto wide = [&](const void *W, void *out, int64_t N, int epi) -> int {
        if (!b->dma) return launch_linear(L, dt, W, sc.xn, nullptr, out, T, N, D.h, epi, sc.inv_rms, 1, nullptr, true);
        GemvBatchArgs ga;
        ga.W = W; ga.x = sc.xn; ga.x_scale = sc.inv_rms; ga.out = out; ga.N = (int)N; ga.K = (int)D.h; ga.epi = epi; ga.pro = PRO_X; ga.B = B; ga.nks = 1;
        return launch_gemv_dma(L, ga);
    };
    const bool ps = b->per_seq;
    const size_t es = m->esize();
    if (ps && !b->plain) { for (int i = 0; i < B; i++) FL_TRY(launch_embed(L, dt, sh.embed, nullptr, b->caches[i]->shards[0].st, sc.x_res + (size_t)i * D.h, 1, D.h)); }
    else FL_TRY(launch_embed_batch(L, sh.embed, b->seqs_dev, sc.x_res, B, D.h, dt));
    const int64_t nq = (sh.Hs + 2 * sh.Hkvs) * D.d;
    // per-sequence mode: row i's RoPE / KV append and attention on the single-sequence kernels (position, length and cache of sequence i)
    auto rope_attn_per_seq = [&](int64_t l, const float *bias) -> int {
        for (int i = 0; i < B; i++) {
            Cache *ci = b->caches[i];
            CacheShard &cs = ci->shards[0];
            const KvLayer kv(m, ci, sh, cs, l);
            void *qi = (char *)sc.q + (size_t)i * sh.Hs * D.d * es, *aoi = (char *)sc.ao + (size_t)i * sh.Hs * D.d * es;
            FL_TRY(launch_rope_kv(L, dt, sc.qkv + (size_t)i * nq, cs.st, sh.cos_tab, sh.sin_tab, D.max_pos, qi, kv.k, kv.v, 1, sh.Hs, sh.Hkvs, D.d, (int64_t)ci->seq_alloc, ci->v_transposed, 1, bias));
            const AttnScratch as{cs.part_m, cs.part_l, cs.part_o, cs.counters, ci->nsplit, 0};
            FL_TRY(attend_decode(L, m, ci, sh, cs, kv, qi, aoi, as));
        }
        return FL_OK;
    };
    // Round 5, FL_GEMM_SKF=2 (off by default: it measured 8-13 % SLOWER, profiles/r05/README.md): the layer as FIVE launches (k_gemm_skf.hip) -- QKV with each row's RoPE / KV append in its epilogue, attention, o_proj and
    // down_proj with the residual + next norm in theirs (K slices met inside the launch: no slabs, no rmsnorm_add), gate/up with its
    // row scales from the partial sums -- where every projection of the model has a plan there; otherwise the eight-launch layer below
    const bool tpr = m->tp > 1;                                        // a rank of a multi-process group: all-reduce behind o_proj / down_proj, gathered logits
    const int ks_q = dt == FL_DTYPE_BF16 && sc.rs_part && !tpr && !ps && tune(TK_GEMM_SKF) >= 2 ? gemm_skf_plan(T, nq, D.h, EPI_QKV_ROPE, (int)D.d) : 0;
    const LinearPlan po = plan_resid(dt, T, D.h, sh.Hs * D.d, 1, true), pd = plan_resid(dt, T, D.h, sh.Ip, 1, true);
    if (ks_q && po.kernel == LK_SKF && pd.kernel == LK_SKF && gemm_skf_plan(T, 2 * sh.Ip, D.h, EPI_GATEUP) > 0) {
        const int np = gemm_resid_partials(D.h);
        auto resid = [&](const LinearPlan &p, const void *W, const void *x, int64_t K, const float *next_w) -> int {
            const ResidEpi re = resid_epi(sc, D, next_w);
            return launch_plan(L, p, dt, W, x, nullptr, nullptr, T, D.h, K, EPI_RESID, nullptr, &re);
        };
        const RsParts parts{sc.rs_part, np, D.eps, 1.0f / (float)D.h};
        FL_TRY(launch_rmsnorm_add(L, dt, sc.x_res, nullptr, sh.layers[0].ln1, D.eps, sc.xn, sc.inv_rms, T, D.h, 1, slab));
        for (int64_t l = 0; l < D.L; l++) {
            LayerW &ly = sh.layers[l];
            RopeEpi ro;
            ro.cos_tab = sh.cos_tab; ro.sin_tab = sh.sin_tab; ro.max_pos = (int)D.max_pos; ro.q_out = sc.q;
            ro.H = (int)sh.Hs; ro.Hkv = (int)sh.Hkvs; ro.d = (int)D.d; ro.v_transposed = 1;
            ro.seqs = b->seqs_dev; ro.kv_layer_off = (size_t)l * sh.Hkvs * D.d;
            if (l > 0) L.rsp = parts;                                    // (the previous layer's down_proj left 1/rms as partial sums)
            FL_TRY(launch_gemm_skf(L, ly.wqkv, sc.xn, ly.bqkv, nullptr, T, nq, D.h, EPI_QKV_ROPE, sc.inv_rms, ks_q, nullptr, &ro));
            L.rsp = RsParts{};
            FL_TRY(launch_attn_decode_mfma_batch(L, sc.q, b->seqs_dev, B, b->max_nsplit, (size_t)l * sh.Hkvs * D.d, sc.ao, sh.Hs, sh.Hkvs,
                                                 D.d, D.scale, 0.0));
            FL_TRY(resid(po, ly.wo, sc.ao, sh.Hs * D.d, ly.ln2));
            if (b->dma) {                                                // (eight rows at most: the LDS-DMA ring kernel streams gate/up fastest, and takes a vector)
                FL_TRY(launch_rms_finalize(L, sc.rs_part, np, D.eps, sc.inv_rms, T, D.h));
                FL_TRY(wide(ly.wgu, sc.act, 2 * sh.Ip, EPI_GATEUP));
            } else {
                L.rsp = parts;
                FL_TRY(launch_linear(L, dt, ly.wgu, sc.xn, nullptr, sc.act, T, 2 * sh.Ip, D.h, EPI_GATEUP, sc.inv_rms, 1, nullptr, true));
                L.rsp = RsParts{};
            }
            FL_TRY(resid(pd, ly.wd, sc.act, sh.Ip, l + 1 < D.L ? sh.layers[l + 1].ln1 : sh.norm));
        }
        FL_TRY(launch_rms_finalize(L, sc.rs_part, np, D.eps, sc.inv_rms, T, D.h));
        FL_TRY(wide(sh.lm_head, b->logits, D.V, EPI_F32));
        return batch_select(b, L, kind);
    }
    for (int64_t l = 0; l < D.L; l++) {
        LayerW &ly = sh.layers[l];
        FL_TRY(launch_rmsnorm_add(L, dt, sc.x_res, l == 0 ? nullptr : sc.delta, ly.ln1, D.eps, sc.xn, sc.inv_rms, T, D.h, nslab, slab));
        // K slices for the QKV stream too (96 strips of 64 rows otherwise: a third of the chip); the bias, if any, moves
        // into the RoPE launch, which sums the slabs anyway
        int qkv_slabs = 1;
        if (b->plain) {
            // plain cache layout (fp32 models; bf16 outside the MFMA attention's head shapes): the batch kernels' plain forms
            FL_TRY(launch_linear(L, dt, ly.wqkv, sc.xn, nullptr, sc.qkv, T, nq, D.h, EPI_F32, sc.inv_rms, 1, nullptr, true));
            FL_TRY(launch_rope_kv_batch(L, sc.qkv, b->seqs_dev, sh.cos_tab, sh.sin_tab, D.max_pos, sc.q, (size_t)l * sh.Hkvs * D.d, B, sh.Hs,
                                        sh.Hkvs, D.d, 1, ly.bqkv, dt, false));
            FL_TRY(launch_attn_decode_batch(L, dt, sc.q, b->seqs_dev, B, b->max_nsplit, (size_t)l * sh.Hkvs * D.d, sc.ao, sh.Hs, sh.Hkvs, D.d, D.scale));
        } else if (ps) {
            FL_TRY(launch_linear(L, dt, ly.wqkv, sc.xn, nullptr, sc.qkv, T, nq, D.h, EPI_F32, sc.inv_rms, 1, nullptr, true));
            FL_TRY(rope_attn_per_seq(l, ly.bqkv));
        } else {
            FL_TRY(launch_linear(L, dt, ly.wqkv, sc.xn, nullptr, sc.qkv, T, nq, D.h, EPI_F32, sc.inv_rms, kMaxQkvSplitShort, &qkv_slabs, true));
            FL_TRY(launch_rope_kv_batch(L, sc.qkv, b->seqs_dev, sh.cos_tab, sh.sin_tab, D.max_pos, sc.q, (size_t)l * sh.Hkvs * D.d, B, sh.Hs,
                                        sh.Hkvs, D.d, qkv_slabs, ly.bqkv));
            FL_TRY(launch_attn_decode_mfma_batch(L, sc.q, b->seqs_dev, B, b->max_nsplit, (size_t)l * sh.Hkvs * D.d, sc.ao, sh.Hs, sh.Hkvs,
                                                 D.d, D.scale, 0.0));
        }
        // (a rank's row-parallel outputs: complete, no slabs -- the all-reduce wants the sum; sums in rank order on every rank)
        FL_TRY(launch_linear(L, dt, ly.wo, sc.ao, nullptr, sc.delta, T, D.h, sh.Hs * D.d, EPI_F32, nullptr, tpr ? 1 : kMaxKSplit, &nslab, true));
        if (tpr) FL_TRY(oneshot(m, sh, false, sc.delta, sc.delta, T * D.h, 0));
        FL_TRY(launch_rmsnorm_add(L, dt, sc.x_res, sc.delta, ly.ln2, D.eps, sc.xn, sc.inv_rms, T, D.h, nslab, slab));
        FL_TRY(wide(ly.wgu, sc.act, 2 * sh.Ip, EPI_GATEUP));
        FL_TRY(launch_linear(L, dt, ly.wd, sc.act, nullptr, sc.delta, T, D.h, sh.Ip, EPI_F32, nullptr, tpr ? 1 : kMaxKSplit, &nslab, true));
        if (tpr) FL_TRY(oneshot(m, sh, false, sc.delta, sc.delta, T * D.h, 0));
    }
    FL_TRY(launch_rmsnorm_add(L, dt, sc.x_res, sc.delta, sh.norm, D.eps, sc.xn, sc.inv_rms, T, D.h, nslab, slab));
    if (tpr) {
        // every rank's [B][V / tp] block of the logits, gathered in one collective (rank-major) and laid out [B][V] for token selection
        FL_TRY(wide(sh.lm_head, b->logits_local, sh.Vs, EPI_F32));
        FL_TRY(oneshot(m, sh, true, b->logits_local, b->logits_ranks, (int64_t)B * sh.Vs, (int64_t)B * sh.Vs));
        FL_TRY(launch_unshard_logits(L, b->logits_ranks, b->logits, m->tp, B, sh.Vs));
    } else {
        FL_TRY(wide(sh.lm_head, b->logits, D.V, EPI_F32));
    }
    return batch_select(b, L, kind);
}

// kind (kStepLp | kStepRules | kStepGuide): the step with every sequence's log-prob records written behind token selection (one more
// launch of B workgroups) and / or the logit-rules and guide launches in front of it, each kind a graph of its own; graph[0] is what it
// always was
static int batch_step(Batch *b, int kind = 0) {
    Model *m = b->m;
    Shard &sh = m->shards[0];
    const bool graphable = m->use_graph && !m->profiling && !b->graph_failed;
    if (!(kind & kStepLp)) return replay_or_capture({{sh.device, sh.stream, &b->graph[kind]}}, graphable, b->graph_failed, b->warm_steps[kind], [b, kind] { return enqueue_batch_step(b, kind); });
    return replay_or_capture({{sh.device, sh.stream, &b->graph[kind]}}, graphable, b->graph_failed, b->warm_steps[kind], [b, m, &sh, kind]() -> int {
        FL_TRY(enqueue_batch_step(b, kind));
        Launcher L = make_launcher(m, sh);
        LogprobSrc src;
        src.seqs = b->seqs_dev; src.ctls = b->lp_ctls;
        return launch_token_logprobs(L, b->logits, m->D.V, b->B, src, 1);
    });
}

// The end of a batch call, per sequence: n_tokens of every cache's token buffer and its StepState come back through the pinned
// buffers, the stream is waited for, and the error words of the collectives and of each sequence are looked at.  with_lp: as many
// log-prob records of every sequence too.
static int batch_finish(Batch *b, size_t n_tokens, bool with_lp = false) {
    Shard &sh = b->m->shards[0];
    for (int i = 0; i < b->B; i++) {
        if (with_lp) FL_HIP(hipMemcpyAsync(b->host_lp + (size_t)i * kBatchChunk, b->caches[i]->shards[0].lp_recs, n_tokens * sizeof(LogprobRec), hipMemcpyDeviceToHost, sh.stream));
        FL_HIP(hipMemcpyAsync(b->host_tokens + (size_t)i * kBatchChunk, b->caches[i]->shards[0].out_tokens, n_tokens * 4, hipMemcpyDeviceToHost, sh.stream));
        FL_HIP(hipMemcpyAsync(b->host_states + i, b->caches[i]->shards[0].st, sizeof(StepState), hipMemcpyDeviceToHost, sh.stream));
    }
    FL_HIP(hipStreamSynchronize(sh.stream));
    FL_TRY(comm_check(b->m));                                 // (a tensor-parallel rank: a collective that gave up waiting for a peer)
    for (int i = 0; i < b->B; i++)
        if (b->host_states[i].error) FL_FAIL(FL_ERR_HIP, "device-side wait gave up (code 0x%x) in sequence %d", b->host_states[i].error, i);
    return FL_OK;
}

static int batch_check(Batch *b, const size_t *pos, size_t n_steps) {
    if (!b || !pos) FL_FAIL(FL_ERR_BAD_ARGUMENT, "null argument");
    for (int i = 0; i < b->B; i++) FL_TRY(check_call(b->m, b->caches[i], n_steps, pos[i]));
    return FL_OK;
}

int batch_decode(Batch *b, const uint32_t *first, const size_t *pos, size_t n_steps, int64_t eos,
                 const fl_sampler *sampling, uint32_t *tokens_out, size_t *n_out) {
    if (!b) FL_FAIL(FL_ERR_BAD_ARGUMENT, "null argument");
    std::vector<int64_t> e((size_t)b->B, eos);
    fl_sampler greedy{};
    greedy.struct_size = sizeof(fl_sampler);
    std::vector<fl_sampler> sp((size_t)b->B, sampling ? *sampling : greedy);
    return batch_decode_each(b, first, pos, n_steps, e.data(), sp.data(), tokens_out, n_out);
}

// ... with every sequence's own EOS id and sampler (a request's temperature is its own: chat.rs:24-25; temperature < 1e-7 = ArgMax)
int batch_decode_each(Batch *b, const uint32_t *first, const size_t *pos, size_t n_steps, const int64_t *eos_each,
                      const fl_sampler *sampling_each, uint32_t *tokens_out, size_t *n_out, const fl_logprobs *lp_each) {
    if (!b || !first || !tokens_out || !n_out) FL_FAIL(FL_ERR_BAD_ARGUMENT, "null argument");
    const int B = b->B;
    if (lp_each) {
        for (int i = 0; i < B; i++) FL_TRY(check_logprobs(lp_each + i, b->m->D.V));
        if (b->m->tp > 1) FL_FAIL(FL_ERR_UNSUPPORTED, "token log-probabilities do not run on a tensor-parallel group's batch (tp_size %d)", b->m->tp);
    }
    for (int i = 0; i < B; i++) n_out[i] = 0;
    if (n_steps == 0) return FL_OK;
    FL_TRY(batch_check(b, pos, n_steps));
    Model *m = b->m;
    for (int i = 0; i < B; i++) FL_TRY(check_token(m, first[i], "token"));
    std::vector<SampleState> samplers((size_t)B);
    std::vector<int64_t> eoss((size_t)B, -1);
    for (int i = 0; i < B; i++) {
        FL_TRY(make_sampler(sampling_each ? sampling_each + i : nullptr, m->D.V, &samplers[(size_t)i]));
        if (eos_each) eoss[(size_t)i] = eos_each[i];
    }
    std::lock_guard<std::mutex> lock(m->mu);
    Shard &sh = m->shards[0];
    FL_HIP(hipSetDevice(sh.device));
    if (lp_each) {
        // every member's record buffer (a replaced slot's cache may not have one yet), the table the step's launch reads them from,
        // and each sequence's top_n -- all ahead of the steps on the stream
        if (!b->lp_ctls) FL_TRY(dev_alloc(b->allocs, (void **)&b->lp_ctls, sizeof(LogprobCtl *) * (size_t)B, nullptr));
        if (!b->host_lp) FL_HIP(hipHostMalloc((void **)&b->host_lp, (size_t)B * kBatchChunk * sizeof(LogprobRec), hipHostMallocDefault));
        std::vector<LogprobCtl *> ctls((size_t)B);
        Launcher L = make_launcher(m, sh);
        for (int i = 0; i < B; i++) {
            FL_TRY(ensure_logprobs(m, b->caches[i]));
            CacheShard &cs = b->caches[i]->shards[0];
            ctls[(size_t)i] = cs.lp_ctl;
            FL_TRY(launch_set_logprob_ctl(L, cs.lp_ctl, cs.lp_recs, (uint32_t)kOutTokensCap, lp_each[i].top_n));
        }
        FL_HIP(hipMemcpy(b->lp_ctls, ctls.data(), sizeof(LogprobCtl *) * (size_t)B, hipMemcpyHostToDevice));   // (synchronous: ctls is a stack vector)
    }
    bool rules = false;
    for (int i = 0; i < B; i++) rules = rules || b->caches[i]->rules_on;
    if (rules) {
        // the adjusted rows and the members' control blocks (null: no rules -- the row is copied through), and each ruled member's
        // scalars with count_input set: every step's input token is one more output -- all ahead of the steps on the stream
        if (!b->rule_ctls) FL_TRY(dev_alloc(b->allocs, (void **)&b->rule_ctls, sizeof(LogitRulesCtl *) * (size_t)B, nullptr));
        if (!b->logits_adj) FL_TRY(dev_alloc(b->allocs, (void **)&b->logits_adj, (size_t)B * m->D.V * 4, nullptr));
        std::vector<LogitRulesCtl *> ctls((size_t)B, nullptr);
        for (int i = 0; i < B; i++) {
            if (!b->caches[i]->rules_on) continue;
            FL_TRY(set_logit_rules_ctl(m, b->caches[i], true));
            ctls[(size_t)i] = b->caches[i]->shards[0].rule_ctl;
        }
        FL_HIP(hipMemcpy(b->rule_ctls, ctls.data(), sizeof(LogitRulesCtl *) * (size_t)B, hipMemcpyHostToDevice));   // (synchronous: ctls is a stack vector)
    }
    bool guided = false;
    for (int i = 0; i < B; i++) guided = guided || b->caches[i]->guide;
    if (guided) {
        // the masked rows and the members' control blocks (null: no guide -- the row is copied through); each guided member's state is
        // written per chunk below
        if (!b->guide_ctls) FL_TRY(dev_alloc(b->allocs, (void **)&b->guide_ctls, sizeof(GuideCtl *) * (size_t)B, nullptr));
        if (!b->logits_guided) FL_TRY(dev_alloc(b->allocs, (void **)&b->logits_guided, (size_t)B * m->D.V * 4, nullptr));
        std::vector<GuideCtl *> ctls((size_t)B, nullptr);
        for (int i = 0; i < B; i++) if (b->caches[i]->guide) ctls[(size_t)i] = b->caches[i]->shards[0].guide_ctl;
        FL_HIP(hipMemcpy(b->guide_ctls, ctls.data(), sizeof(GuideCtl *) * (size_t)B, hipMemcpyHostToDevice));   // (synchronous: ctls is a stack vector)
    }
    const int kind = (lp_each ? kStepLp : 0) | (rules ? kStepRules : 0) | (guided ? kStepGuide : 0);
    std::vector<uint32_t> tok(first, first + B);
    std::vector<char> finished(B, 0);
    std::vector<size_t> len0(B);
    for (int i = 0; i < B; i++) len0[i] = b->caches[i]->len;
    size_t done = 0;
    while (done < n_steps) {
        const size_t nb = std::min(n_steps - done, kBatchChunk);
        for (int i = 0; i < B; i++)
            FL_TRY(set_shard_state(m, sh, b->caches[i]->shards[0], tok[i], pos[i] + done, len0[i] + done, len0[i] + done, 0u, eoss[(size_t)i], samplers[(size_t)i], done == 0));
        for (int i = 0; i < B; i++)
            if (b->caches[i]->guide) FL_TRY(set_guide_ctl(m, b->caches[i]));   // the host's state: the device advances it inside the chunk
        for (size_t s = 0; s < nb; s++) FL_TRY(batch_step(b, kind));
        FL_TRY(batch_finish(b, nb, lp_each != nullptr));
        bool all_finished = true;
        for (int i = 0; i < B; i++) {
            if (!finished[i]) {
                for (size_t s = 0; s < nb; s++) {
                    const uint32_t t = b->host_tokens[(size_t)i * kBatchChunk + s];
                    if (const Guide *g = b->caches[i]->guide) b->caches[i]->guide_state = g->walk(b->caches[i]->guide_state, t);   // (the EOS's edge too; the walk stops there)
                    if (eoss[(size_t)i] >= 0 && (int64_t)t == eoss[(size_t)i]) {   // as fl_decode_greedy: the EOS forward counts, the token does not
                        finished[i] = 1;
                        b->caches[i]->len = len0[i] + done + s + 1;
                        break;
                    }
                    tokens_out[(size_t)i * n_steps + done + s] = t;
                    if (lp_each) scatter_logprobs(b->host_lp[(size_t)i * kBatchChunk + s], lp_each + i, done + s);
                    n_out[i] = done + s + 1;
                }
                if (!finished[i]) b->caches[i]->len = len0[i] + done + nb;
            }
            tok[i] = b->host_tokens[(size_t)i * kBatchChunk + nb - 1];
            all_finished = all_finished && finished[i];
        }
        done += nb;
        if (all_finished) break;
    }
    return FL_OK;
}

int batch_forward(Batch *b, const uint32_t *tokens, const size_t *pos, float *logits_out, uint32_t *tokens_out) {
    if (!b || !tokens) FL_FAIL(FL_ERR_BAD_ARGUMENT, "null argument");
    FL_TRY(batch_check(b, pos, 1));
    Model *m = b->m;
    const int B = b->B;
    for (int i = 0; i < B; i++) FL_TRY(check_token(m, tokens[i], "token"));
    if (tokens_out) for (int i = 0; i < B; i++) {                    // (its ArgMax reads the raw rows)
        FL_TRY(refuse_logit_rules(b->caches[i], "fl_batch_forward with argmax_out"));
        FL_TRY(refuse_guide(b->caches[i], "fl_batch_forward with argmax_out"));
    }
    const SampleState sampler{};
    std::lock_guard<std::mutex> lock(m->mu);
    Shard &sh = m->shards[0];
    FL_HIP(hipSetDevice(sh.device));
    for (int i = 0; i < B; i++)
        FL_TRY(set_shard_state(m, sh, b->caches[i]->shards[0], tokens[i], pos[i], b->caches[i]->len, b->caches[i]->len, 0u, -1, sampler, true));
    FL_TRY(batch_step(b));
    if (logits_out) FL_HIP(hipMemcpyAsync(logits_out, b->logits, (size_t)B * m->D.V * 4, hipMemcpyDeviceToHost, sh.stream));
    FL_TRY(batch_finish(b, 1));
    for (int i = 0; i < B; i++) {
        b->caches[i]->len += 1;
        if (tokens_out) tokens_out[i] = b->host_tokens[(size_t)i * kBatchChunk];
    }
    return FL_OK;
}

}  // namespace fl
