// model.hip -- KV cache and the per-layer orchestration of the decoder forward pass on MI355X.
//
// Reference semantics reproduced here (all citations into /root/reference/src/models):
//   forward(input, pos, cache)     llama.rs:147-149, mistral.rs:206-236, qwen.rs:123-151
// The arithmetic follows candle 0.8.x.
//   KV cache [L][Hkvs][max_seq][d] x2, written in place (no Tensor::cat copy)
#include "model.h"
#include "lookup.h"

#include <math.h>

#include <algorithm>
#include <memory>

namespace fl {

// ------------------------------------------------------------------------------- cache
// Decode attention's split count for a cache of max_seq positions (v_transposed: the MFMA kernels' layout).
int attn_cache_nsplit(bool v_transposed, size_t max_seq, int64_t d) {
    // decode attention splits S so that the K/V stream of one kv head is spread over many CUs
    // (~64 cached positions per 4-wave workgroup at full length); partials are combined in-launch
    // MFMA kernel: 128 keys (four 32-key wave steps) per workgroup; VALU kernel: 64.  One CU pulls only
    // ~25-50 GB/s from HBM, so a kv head's K/V stream must be spread over many CUs -- except when it is
    // small (<= 96 KB per head): then one wide workgroup per head with no cross-workgroup combine wins.
    // Long caches: 256 keys (two steps per wave) -- fewer workgroups and half the partials to combine.  A/B inside one process
    // (tools/decode_ab.py, FL_ATTN_NSPLIT, tokens/s): Qwen2-7B at S = 4100 34 / 24 / 17 / 12 splits 361.3 / 363.1 / 364.9 / 359.6,
    // Mistral-7B at S = 4100 34 / 17 splits 340.5 / 347.1, at S = 2100 18 / 9 splits 358.0 / 356.9, at S = 530 7 / 4 370.4 / 364.5.
    // (A workgroup never takes fewer than 128 keys, so the split count of a large cache costs a short sequence nothing.)
    const int64_t keys_per_wg = v_transposed ? (max_seq > 2560 ? 256 : 128) : 64;
    int64_t ns = (int64_t)((max_seq + keys_per_wg - 1) / keys_per_wg);
    if (v_transposed && max_seq * (size_t)d * 4 <= 96 * 1024) ns = 1;
    return (int)std::max<int64_t>(1, std::min<int64_t>(ns, v_transposed ? 48 : 64));   // (measured at S = 8192 / 16384: 32..48 splits 17.4 / 24.0 us, 64: 18.7 / 25.4)
}

Cache::~Cache() {
    if (!m) return;
    {
        std::lock_guard<std::mutex> lock(m->mu);   // not while another thread captures on the model's stream
        for (size_t i = 0; i < shards.size(); i++) {
            (void)hipSetDevice(m->shards[i].device);
            (void)hipStreamSynchronize(m->shards[i].stream);
            for (auto g : shards[i].graph) if (g) (void)hipGraphExecDestroy(g);
            for (void *p : shards[i].allocs) (void)hipFree(p);
            if (shards[i].rule_image) (void)hipHostFree(shards[i].rule_image);
        }
    }
    if (guide) guide_release(guide);               // (outside the lock: the last reference frees the device copy under it)
}

int cache_create(Model *m, size_t max_seq, Cache **out) {
    if (!m || !out) FL_FAIL(FL_ERR_BAD_ARGUMENT, "null argument");
    if (max_seq == 0) FL_FAIL(FL_ERR_BAD_ARGUMENT, "max_seq must be > 0");
    debug_inject("cache_create");
    const Dims &D = m->D;
    std::unique_ptr<Cache> c(new Cache());
    c->m = m; c->max_seq = max_seq; c->len = 0;
    // Under the model mutex and on the model's stream: another thread may be capturing its decode graph
    // on that stream, and a legacy-stream memset would try to join the capture.
    std::lock_guard<std::mutex> lock(m->mu);
    c->seq_alloc = (max_seq + 31) / 32 * 32;
    c->v_transposed = tune(TK_ATTN_MFMA) != 0 && attn_mfma_supported(m->dtype, m->shards[0].Hs, m->shards[0].Hkvs, D.d);
    c->nsplit = attn_cache_nsplit(c->v_transposed, max_seq, D.d);
    if (tune(TK_ATTN_NSPLIT) >= 0) c->nsplit = tune(TK_ATTN_NSPLIT);
    {   // decode attention + o_proj in one launch when W_o's per-CU slice fits in LDS next to the attention state
        hipDeviceProp_t prop;
        FL_HIP(hipGetDeviceProperties(&prop, m->shards[0].device));
        // the fused launch's attention workgroups take 32 keys per wave and step; of their eight waves as few take keys as
        // keeps the splits few enough (a CU pulls only ~40 GB/s, so a split's K/V should stay small -- but every split
        // is a workgroup that holds no rows of W_o, and the others' LDS is full at ~156 rows)
        const int cus = prop.multiProcessorCount;
        const int w0 = tune(TK_AO_WAVES);
        c->fuse_oproj = false;
        for (int aw = w0 > 0 ? std::min(w0, 8) : 4; aw <= (w0 > 0 ? std::min(w0, 8) : 8) && !c->fuse_oproj; aw++) {
            const int ns8 = (int)std::max<int64_t>(1, (int64_t)((max_seq + 32 * aw - 1) / (32 * aw)));
            int nb = 0, ra = 0, ro = 0; size_t lds;
            const bool fits = m->fused_decode && c->v_transposed && m->tp == 1 && m->shards.size() == 1 && !m->shards[0].comm &&
                              attn_oproj_plan(m->shards[0].Hs, m->shards[0].Hkvs, D.d, D.h, ns8, cus, &nb, &ra, &ro, &lds);
            // where it pays (profiles/r02/README.md): the workgroups of a kv head are the 32 of one XCD (8 kv heads on 256 CUs)
            // and the attention workgroups own next to no rows, i.e. short contexts of Mistral-like shapes; TinyLlama / Qwen2
            // (4 kv heads: groups of 64 over two XCDs) and long contexts are faster as two launches
            const bool pays = fits && cus / m->shards[0].Hkvs <= 32 && ra <= 16;
            c->fuse_oproj = m->fuse_oproj > 0 ? fits : (m->fuse_oproj < 0 ? pays : false);
            if (m->decode_weights != FL_WEIGHTS_COMPUTE_DTYPE) c->fuse_oproj = false;     // (that launch streams the bf16 wo itself)
            c->ao_nsplit = ns8; c->ao_waves = aw;
        }
    }
    // short caches: attention replicated in every workgroup of the o_proj launch (k_attn_rep.hip): one launch and one dependent
    // step fewer per layer; FL_ATTN_REP=0 keeps the two launches
    c->rep_attn = tune(TK_ATTN_REP) != 0 && m->fused_decode && c->v_transposed && !c->fuse_oproj && m->dtype == FL_DTYPE_BF16 &&
                  m->decode_weights == FL_WEIGHTS_COMPUTE_DTYPE &&       // (k_attn_rep.hip streams the bf16 wo itself)
                  attn_oproj_rep_supported(m->shards[0].Hs, m->shards[0].Hkvs, D.d, D.h, (int64_t)c->seq_alloc, tune(TK_ATTN_REP) == 2);
    c->shards.resize(m->shards.size());
    for (size_t i = 0; i < m->shards.size(); i++) {
        Shard &sh = m->shards[i]; CacheShard &cs = c->shards[i];
        FL_HIP(hipSetDevice(sh.device));
        const size_t kvb = (size_t)D.L * sh.Hkvs * c->seq_alloc * D.d * m->esize();
        FL_TRY(dev_alloc(cs.allocs, &cs.k, kvb, nullptr));
        FL_TRY(dev_alloc(cs.allocs, &cs.v, kvb, nullptr));
        // finite contents everywhere: the MFMA kernel multiplies masked keys' values by p = 0
        FL_HIP(hipMemsetAsync(cs.k, 0, kvb, sh.stream));
        FL_HIP(hipMemsetAsync(cs.v, 0, kvb, sh.stream));
        FL_TRY(dev_alloc(cs.allocs, (void **)&cs.st, sizeof(StepState), nullptr));
        FL_TRY(dev_alloc(cs.allocs, (void **)&cs.out_tokens, kOutTokensCap * 4, nullptr));
        FL_TRY(dev_alloc(cs.allocs, (void **)&cs.part_m, (size_t)sh.Hs * c->nsplit * 4, nullptr));
        FL_TRY(dev_alloc(cs.allocs, (void **)&cs.part_l, (size_t)sh.Hs * c->nsplit * 4, nullptr));
        FL_TRY(dev_alloc(cs.allocs, (void **)&cs.part_o, (size_t)sh.Hs * c->nsplit * D.d * 4, nullptr));
        FL_TRY(dev_alloc(cs.allocs, (void **)&cs.counters, (size_t)sh.Hs * 4, nullptr));
        FL_HIP(hipMemsetAsync(cs.counters, 0, (size_t)sh.Hs * 4, sh.stream));
        FL_TRY(dev_alloc(cs.allocs, (void **)&cs.ss, sizeof(SampleState), nullptr));
        FL_HIP(hipMemsetAsync(cs.ss, 0, sizeof(SampleState), sh.stream));
        FL_TRY(dev_alloc(cs.allocs, (void **)&cs.sel_scratch, (size_t)D.V * 4, nullptr));
        if (c->fuse_oproj) {
            FL_TRY(dev_alloc(cs.allocs, (void **)&cs.ao_part, (size_t)sh.Hs * c->ao_nsplit * (D.d + 4) * 4, nullptr));
        }
        FL_TRY(dev_alloc(cs.allocs, (void **)&cs.heads_done, (size_t)D.L * sh.Hkvs * 4, nullptr));
        FL_HIP(hipMemsetAsync(cs.heads_done, 0, (size_t)D.L * sh.Hkvs * 4, sh.stream));
        FL_HIP(hipMemsetAsync(cs.st, 0, sizeof(StepState), sh.stream));
        FL_HIP(hipStreamSynchronize(sh.stream));
    }
    m->refs.fetch_add(1);
    *out = c.release();
    return FL_OK;
}

// ------------------------------------------------------------------------------- forward
__global__ void set_state_kernel(StepState *st, uint32_t token, uint32_t pos, uint32_t len, uint32_t call0, uint32_t step, int32_t eos,
                                 unsigned *heads_done, int n_layers, SampleState *ss, SampleState ss_new, int ss_set) {
    if (threadIdx.x == 0) {
        st->token = token; st->pos = pos; st->len = len; st->call0 = call0; st->step = step; st->eos = eos; st->done = 0; st->error = 0;
        if (ss_set) *ss = ss_new;
    }
    for (int l = threadIdx.x; l < n_layers; l += blockDim.x) heads_done[l] = 0;       // targets restart with step
}

int set_shard_state(Model *m, Shard &sh, CacheShard &cs, uint32_t token, size_t pos, size_t len, size_t call0, uint32_t step, int64_t eos, const SampleState &ss_new, bool ss_set) {
    hipLaunchKernelGGL(set_state_kernel, dim3(1), dim3(64), 0, sh.stream, cs.st, token, (uint32_t)pos, (uint32_t)len, (uint32_t)call0, step,
                       (int32_t)eos, cs.heads_done, (int)(m->D.L * sh.Hkvs), cs.ss, ss_new, ss_set ? 1 : 0);
    FL_HIP(hipGetLastError());
    return FL_OK;
}

// LogitsProcessor::new(seed, Some(temperature), top_p) / from_sampling (mod.rs:373-374): ArgMax below 1e-7, else the
// StdRng stream of rand 0.8 -- ChaCha12 keyed by SeedableRng::seed_from_u64 (PCG32 XSH-RR expansion of
// the u64 into 8 little-endian key words) -- positioned after `draws_done` u32 words.  top_p outside (0, 1) and
// top_k == 0 or >= V are "off" (Sampling::All), as in candle [UPSTREAM-RECALLED]; V <= 0: the vocabulary is not known
// here, any positive top_k is kept (a top_k >= V keeps everything in the kernel too).
int make_sampler(const fl_sampler *sp, int64_t V, SampleState *out) {
    SampleState s{};
    *out = s;
    if (!sp) return FL_OK;
    if (sp->struct_size != sizeof(fl_sampler)) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_sampler.struct_size is %u, expected %zu", sp->struct_size, sizeof(fl_sampler));
    if (sp->top_p != sp->top_p) FL_FAIL(FL_ERR_BAD_ARGUMENT, "top_p is NaN");
    if (sp->top_k < 0) FL_FAIL(FL_ERR_BAD_ARGUMENT, "negative top_k %d", sp->top_k);
    if (!(sp->temperature >= 1e-7)) return FL_OK;
    s.on = tune(TK_SAMPLE_WALK) ? 2 : 1;       // 2: plain one-lane walk instead of ordered_sum (cross-check)
    s.inv_temp = (float)(1.0 / sp->temperature);
    uint64_t state = sp->seed;
    for (int i = 0; i < 8; i++) {
        state = state * 6364136223846793005ull + 11634580027462260723ull;
        const uint32_t xs = (uint32_t)(((state >> 18) ^ state) >> 27), rot = (uint32_t)(state >> 59);
        s.key[i] = (xs >> rot) | (xs << ((32 - rot) & 31));
    }
    s.draw_lo = (uint32_t)sp->draws_done; s.draw_hi = (uint32_t)(sp->draws_done >> 32);
    const bool p_on = sp->top_p > 0.0 && sp->top_p < 1.0;
    const bool k_on = sp->top_k > 0 && (V <= 0 || (int64_t)sp->top_k < V);
    s.filter = (p_on || k_on) ? 1 : 0;
    s.top_p = p_on ? (float)sp->top_p : INFINITY;          // compared as (f32)top_p
    s.top_k = k_on ? (uint32_t)sp->top_k : 0xffffffffu;
    *out = s;
    return FL_OK;
}

Launcher make_launcher(Model *m, Shard &sh) {
    Launcher L; L.stream = sh.stream; L.prof = m->profiling ? &m->prof : nullptr; L.tp = m->tp; return L;
}

// all-reduce(sum) of each local shard's `delta` [count] fp32 (after o_proj / down_proj rows)
static int all_reduce_delta(Model *m, bool pre, int64_t count) {
    if (m->tp == 1 && !m->shards[0].comm) return FL_OK;
    if (m->tp_mode == FL_TP_EMULATED) {
        std::vector<float *> ptrs;
        for (auto &sh : m->shards) ptrs.push_back(pre ? sh.pre.delta : sh.dec.delta);
        Shard &s0 = m->shards[0];
        FL_HIP(hipSetDevice(s0.device));
        float **tab = m->emu_ptrs + (pre ? m->tp : 0);
        FL_HIP(hipMemcpyAsync(tab, ptrs.data(), sizeof(float *) * m->tp, hipMemcpyHostToDevice, s0.stream));
        FL_HIP(hipStreamSynchronize(s0.stream));          // ptrs is a stack vector
        Launcher L = make_launcher(m, s0);
        return launch_reduce_shards(L, tab, m->tp, count);
    }
    if (m->tp_mode == FL_TP_SINGLE_PROCESS) {
        Shard &s0 = m->shards[0];
        if (s0.pc.connected && (count <= s0.pc.nmax || !s0.comm)) {
            for (auto &sh : m->shards) {
                FL_HIP(hipSetDevice(sh.device));
                float *buf = pre ? sh.pre.delta : sh.dec.delta;
                FL_TRY(oneshot(m, sh, false, buf, buf, count, 0));
            }
            return FL_OK;
        }
    } else if (m->tp_mode == FL_TP_MULTI_PROCESS || m->shards[0].pc.connected) {
        Shard &sh = m->shards[0];
        float *buf = pre ? sh.pre.delta : sh.dec.delta;
        if (sh.pc.connected && (count <= sh.pc.nmax || !sh.comm)) return oneshot(m, sh, false, buf, buf, count, 0);
        if (!sh.comm) FL_FAIL(FL_ERR_RCCL, "tensor-parallel group is not connected: call fl_comm_ipc_connect first");
    }
    FL_NCCL(ncclGroupStart());
    for (auto &sh : m->shards) {
        float *buf = pre ? sh.pre.delta : sh.dec.delta;
        FL_NCCL(ncclAllReduce(buf, buf, (size_t)count, ncclFloat, ncclSum, sh.comm, sh.stream));
    }
    FL_NCCL(ncclGroupEnd());
    return FL_OK;
}

// where a shard's lm_head launch writes: its slice of a sharded vocabulary (gathered below), else the full logits at once
// (a 128 KB device-to-device copy per decode step used to stand here)
static float *lm_head_out(Model *m, Shard &sh) { return m->vocab_parallel ? sh.logits_local : sh.logits_full; }

static int gather_logits(Model *m) {
    if (!m->vocab_parallel) return FL_OK;
    if (m->tp_mode == FL_TP_EMULATED) {
        Shard &s0 = m->shards[0];
        FL_HIP(hipSetDevice(s0.device));
        for (auto &dst : m->shards)
            for (auto &src : m->shards)
                FL_HIP(hipMemcpyAsync(dst.logits_full + src.v0, src.logits_local, (size_t)src.Vs * 4, hipMemcpyDeviceToDevice, s0.stream));
        return FL_OK;
    }
    if (m->tp_mode == FL_TP_SINGLE_PROCESS && m->shards[0].pc.connected && (m->shards[0].Vs <= m->shards[0].pc.nmax || !m->shards[0].comm)) {
        for (auto &sh : m->shards) {
            FL_HIP(hipSetDevice(sh.device));
            FL_TRY(oneshot(m, sh, true, sh.logits_local, sh.logits_full, sh.Vs, sh.Vs));
        }
        return FL_OK;
    }
    if (m->tp_mode == FL_TP_MULTI_PROCESS) {
        Shard &sh = m->shards[0];
        if (sh.pc.connected && (sh.Vs <= sh.pc.nmax || !sh.comm)) return oneshot(m, sh, true, sh.logits_local, sh.logits_full, sh.Vs, sh.Vs);
        if (!sh.comm) FL_FAIL(FL_ERR_RCCL, "tensor-parallel group is not connected: call fl_comm_ipc_connect first");
    }
    FL_NCCL(ncclGroupStart());
    for (auto &sh : m->shards)
        FL_NCCL(ncclAllGather(sh.logits_local, sh.logits_full, (size_t)sh.Vs, ncclFloat, sh.comm, sh.stream));
    FL_NCCL(ncclGroupEnd());
    return FL_OK;
}

static bool fused_all_reduce(Model *m, Cache *c) { return !c->fuse_oproj && fused_all_reduce_ready(m); }

// The decode step on the persistent engine (k_engine.hip): per layer the attention launch and ONE launch that chains
// o_proj -> gate/up -> down_proj -> the next layer's QKV projection (the last layer: lm_head) -- 2 L + 1 launches instead of 5 L + 1.
// One shard, no tensor parallelism (stage 1), bf16, MFMA attention; FL_ENGINE=1 turns it on (default off: see below).
static bool engine_usable(Model *m, Cache *c) {
    const int want = m->engine;
    if (want == 0 || m->shards.size() != 1 || m->tp != 1 || m->dtype != FL_DTYPE_BF16 || !m->fused_decode || c->fuse_oproj || !c->v_transposed) return false;
    if (m->decode_weights != FL_WEIGHTS_COMPUTE_DTYPE) return false;
    Shard &sh = m->shards[0];
    if (!sh.eng_epoch || sh.pc.shares_device || m->D.L < 1) return false;
    if (!gemv_norm_supported(m->dtype, (sh.Hs + 2 * sh.Hkvs) * m->D.d, m->D.h)) return false;
    // opt-in: measured 5 % SLOWER than the five launches it replaces on TinyLlama-1.1B (24.4 us against 23.2 us per layer for
    // o_proj .. QKV; profiles/r03/README.md has the in-kernel stamps: every chip-wide edge costs 2.2-3 us, a kernel boundary
    // + ramp 2.5-3, and the prefetch across an edge only moves the pipeline's fill bubble behind the barrier)
    return want == 1;
}

// fn(sh, cs, L) on every local shard in index order, its device current and L its launcher; stops at the first error
template <typename Fn>
static int each_shard(Model *m, Cache *c, Fn fn) {
    for (size_t i = 0; i < m->shards.size(); i++) {
        Shard &sh = m->shards[i];
        FL_HIP(hipSetDevice(sh.device));
        Launcher L = make_launcher(m, sh);
        FL_TRY(fn(sh, c->shards[i], L));
    }
    return FL_OK;
}

int attend_decode(Launcher &L, const Model *m, const Cache *c, const Shard &sh, const CacheShard &cs, const KvLayer &kv, const void *q, void *ao, const AttnScratch &as) {
    const Dims &D = m->D;
    if (c->v_transposed) return launch_attn_decode_mfma(L, q, kv.k, kv.v, cs.st, ao, as, sh.Hs, sh.Hkvs, D.d, (int64_t)c->seq_alloc, D.scale);
    return launch_attn_decode(L, m->dtype, q, kv.k, kv.v, cs.st, ao, as, sh.Hs, sh.Hkvs, D.d, (int64_t)c->seq_alloc, D.scale);
}

// prefill attention of T new rows (q and the output in the shard's prefill-shaped scratch sc), by the cache's layout likewise
static int attend_prefill(Launcher &L, const Model *m, const Cache *c, const Shard &sh, const CacheShard &cs, const KvLayer &kv, const Scratch &sc, int64_t T) {
    const Dims &D = m->D;
    if (c->v_transposed) return launch_attn_prefill_mfma(L, sc.q, kv.k, kv.v, cs.st, sc.ao, T, sh.Hs, sh.Hkvs, D.d, (int64_t)c->seq_alloc, D.scale, D.window);
    return launch_attn_prefill(L, m->dtype, sc.q, kv.k, kv.v, cs.st, sc.ao, T, sh.Hs, sh.Hkvs, D.d, (int64_t)c->seq_alloc, D.scale, D.window);
}

// The QKV projection of layer l of a decode step on one shard (k_gemv.hip / k_gemv_w8.hip): RMSNorm prologue over the token's
// embedding row (layer 0) or x_res + delta, RoPE + KV append into the layer's caches as the epilogue.
static GemvArgs qkv_gemv_args(Model *m, Cache *c, Shard &sh, CacheShard &cs, const KvLayer &kv, int64_t l) {
    const Dims &D = m->D;
    Scratch &sc = sh.dec; LayerW &ly = sh.layers[l];
    GemvArgs a;
    a.W = ly.wqkv; a.bias = ly.bqkv; a.N = (int)((sh.Hs + 2 * sh.Hkvs) * D.d); a.K = (int)D.h;
    a.epi = EPI_QKV_ROPE; a.pro = PRO_NORM; a.norm_w = ly.ln1; a.eps = D.eps; a.st = cs.st;
    if (l == 0) { a.embed = sh.embed; a.x_out = sc.x_res2; }
    else { a.x_in = sc.x_res; a.delta = sc.delta; a.x_out = sc.x_res2; }
    a.cos_tab = sh.cos_tab; a.sin_tab = sh.sin_tab; a.q_out = sc.q; a.k_cache = kv.k; a.v_cache = kv.v;
    a.H = (int)sh.Hs; a.Hkv = (int)sh.Hkvs; a.d = (int)D.d; a.max_seq = (int)c->seq_alloc; a.max_pos = (int)D.max_pos;
    a.v_ld = c->v_transposed ? (int)c->seq_alloc : 0;
    return a;
}

// A consumer behind a norm takes the vector its producer's residual epilogue finished (GemvArgs: PRO_XS) instead of x_in + delta
static void take_finished_norm(GemvArgs &a, const Scratch &sc) {
    a.pro = PRO_XS; a.x = sc.xs_res; a.cs = sc.cs_res;
    a.x_in = nullptr; a.delta = nullptr; a.delta_nslab = 1; a.norm_w = nullptr; a.x_out = nullptr;
}

static int enqueue_decode_engine(Model *m, Cache *c, int64_t len_hint) {
    const Dims &D = m->D;
    const int dt = m->dtype;
    Shard &sh = m->shards[0]; Scratch &sc = sh.dec; CacheShard &cs = c->shards[0];
    FL_HIP(hipSetDevice(sh.device));
    Launcher L = make_launcher(m, sh);
    const long long timeout_ticks = (long long)tune(TK_ENGINE_TIMEOUT_MS) * 100000ll;
    for (int64_t l = 0; l < D.L; l++) {
        LayerW &ly = sh.layers[l];
        const KvLayer kv(m, c, sh, cs, l);
        if (l == 0) FL_TRY(launch_gemv(L, dt, qkv_gemv_args(m, c, sh, cs, kv, 0)));   // the first QKV projection reads the token's embedding row: the launch of k_gemv.hip
        AttnScratch as{cs.part_m, cs.part_l, cs.part_o, cs.counters, c->nsplit, len_hint + 1};
        FL_TRY(attend_decode(L, m, c, sh, cs, kv, sc.q, sc.ao, as));             // (always the MFMA layout: engine_usable)
        const bool last = l + 1 == D.L;
        float *res_in = (l & 1) ? sc.x_res : sc.x_res2, *res_out = (l & 1) ? sc.x_res2 : sc.x_res;
        EngArgs e;
        e.nops = 4; e.h = (int)D.h; e.x_res_in = res_in; e.eps = D.eps; e.st = cs.st; e.st_rw = cs.st; e.epoch = sh.eng_epoch;
        e.timeout_ticks = timeout_ticks;
        const int t0 = (int)(4 * l);
        EngOp &o0 = e.op[0], &o1 = e.op[1], &o2 = e.op[2], &o3 = e.op[3];
        o0.W = ly.wo; o0.N = (int)D.h; o0.K = (int)(sh.Hs * D.d); o0.in = ENG_IN_X; o0.x = sc.ao; o0.out = ENG_OUT_EDGE_F32; o0.out_edge = sh.eng_edge[0]; o0.tag_out = t0 + 1;
        o1.W = ly.wgu; o1.N = (int)(2 * sh.Ip); o1.K = (int)D.h; o1.in = ENG_IN_NORM; o1.norm_w = ly.ln2; o1.in_edge = sh.eng_edge[0]; o1.tag_in = t0 + 1;
        o1.out = ENG_OUT_EDGE_ACT; o1.out_edge = sh.eng_edge[1]; o1.tag_out = t0 + 2;
        o2.W = ly.wd; o2.N = (int)D.h; o2.K = (int)sh.Ip; o2.in = ENG_IN_ACT; o2.in_edge = sh.eng_edge[1]; o2.tag_in = t0 + 2;
        o2.out = ENG_OUT_EDGE_F32; o2.out_edge = sh.eng_edge[2]; o2.tag_out = t0 + 3;
        o3.K = (int)D.h; o3.in = ENG_IN_NORM; o3.in_edge = sh.eng_edge[2]; o3.tag_in = t0 + 3;
        if (!last) {
            LayerW &nx = sh.layers[l + 1];
            const KvLayer next(m, c, sh, cs, l + 1);
            o3.W = nx.wqkv; o3.N = (int)((sh.Hs + 2 * sh.Hkvs) * D.d); o3.norm_w = nx.ln1; o3.bias = nx.bqkv; o3.out = ENG_OUT_QKV; o3.res_out = res_out;
            e.cos_tab = sh.cos_tab; e.sin_tab = sh.sin_tab; e.q_out = sc.q; e.k_cache = next.k; e.v_cache = next.v;
            e.H = (int)sh.Hs; e.Hkv = (int)sh.Hkvs; e.d = (int)D.d; e.max_seq = (int)c->seq_alloc; e.max_pos = (int)D.max_pos; e.v_ld = (int)c->seq_alloc;
        } else {
            o3.W = sh.lm_head; o3.N = (int)sh.Vs; o3.norm_w = sh.norm; o3.out = ENG_OUT_LOGITS; o3.dst = sh.logits_full;
            if (tune(TK_ARGMAX_FUSED)) { e.amax = sh.amax; sh.amax_valid = true; }
        }
        FL_TRY(launch_engine(L, e));
    }
    return FL_OK;
}

static int enqueue_decode_fused(Model *m, Cache *c, int64_t len_hint) {
    if (engine_usable(m, c)) return enqueue_decode_engine(m, c, len_hint);
    const Dims &D = m->D;
    const int dt = m->dtype;
    const bool far = fused_all_reduce(m, c);
    // FL_WEIGHTS_E4M3_ROW (one shard, bf16: model_create): all six projections stream the e4m3 bytes (k_gemv_w8.hip)
    const bool w8 = m->decode_weights == FL_WEIGHTS_E4M3_ROW;
    auto gemv = [&](Launcher &L, GemvArgs &a, const uint8_t *q8, const float *s8) -> int {
        if (!w8) return launch_gemv(L, dt, a);
        a.W = q8;
        return launch_gemv_w8(L, a, s8);
    };
    auto plain_w8 = [&](Launcher &L, const uint8_t *q8, const float *s8, const void *x, int64_t K, float *out) -> int {
        GemvArgs a;
        a.W = q8; a.x = x; a.out = out; a.N = (int)D.h; a.K = (int)K; a.epi = EPI_F32; a.pro = PRO_X;
        return launch_gemv_w8(L, a, s8);
    };
    // out = sum over ranks of W[h, K] . x  -- the row-parallel projection with the exchange in its epilogue
    auto row_parallel = [&](Launcher &L, Shard &sh, const void *W, const void *x, int64_t K, float *out, int slot) -> int {
        GemvArgs a;
        a.W = W; a.x = x; a.out = out; a.N = (int)D.h; a.K = (int)K; a.epi = EPI_F32; a.pro = PRO_X;
        a.ll = sh.pc.ll_dev; a.ll_slot = slot;
        return launch_gemv(L, dt, a);
    };
    // The two norm edges of a layer (fl_tune "gemv_resid"), decided edge by edge (gemv_resid_edge, gemv_geometry.h): the producer --
    // o_proj / down_proj as a plain launch_gemv -- finishes h = res_in + W . x, h * w_next and the chunk sums of squares in its
    // epilogue, and the consumer stages that vector.  res_in / res_out: the buffers the norm prologue of the edge's consumer reads as
    // x_in and writes as x_out, so that an edge in either form leaves the residual where the next one looks for it.
    const bool resid = tune(TK_GEMV_RESID) != 0 && !far;
    auto edge_fits = [&](int64_t K, int64_t Nc) -> bool {
        return resid && gemv_resid_edge_fits(dt, m->shards.size() == 1 && m->tp == 1, !w8, D.h, K, Nc);
    };
    auto producer = [&](Launcher &L, Scratch &sc, const void *W, const void *x, int64_t K, const float *res_in, float *res_out, const float *w_next) -> int {
        GemvArgs a;
        a.W = W; a.x = x; a.N = (int)D.h; a.K = (int)K; a.epi = EPI_RESID; a.pro = PRO_X;
        a.x_in = res_in; a.norm_w = w_next; a.x_out = res_out; a.xs_out = sc.xs_res; a.cs_out = sc.cs_res;
        return launch_gemv(L, dt, a);
    };
    bool down_done = false;                                  // the previous layer's down_proj has finished this layer's first norm
    for (int64_t l = 0; l < D.L; l++) {
        bool o_done = false;
        FL_TRY(each_shard(m, c, [&](Shard &sh, CacheShard &cs, Launcher &L) -> int {
            Scratch &sc = sh.dec; LayerW &ly = sh.layers[l];
            const KvLayer kv(m, c, sh, cs, l);
            GemvArgs a = qkv_gemv_args(m, c, sh, cs, kv, l);
            if (down_done) take_finished_norm(a, sc);
            FL_TRY(gemv(L, a, ly.wqkv8, ly.sqkv));
            AttnScratch as{cs.part_m, cs.part_l, cs.part_o, cs.counters, c->nsplit, len_hint + 1};
            if (!w8) {
                as.prefetch = ly.wo; as.prefetch_bytes = D.h * sh.Hs * D.d * (int64_t)m->esize();   // o_proj's weights, while HBM idles under the attention
                as.prefetch_chunk = gemv_owner_chunk(dt, D.h, sh.Hs * D.d); as.prefetch_row = sh.Hs * D.d * (int64_t)m->esize();
            }
            if (c->fuse_oproj) {
                FL_TRY(launch_attn_oproj(L, sc.q, kv.k, kv.v, cs.st, cs.st, cs.ao_part, cs.heads_done + l * sh.Hkvs, c->ao_nsplit, c->ao_waves, len_hint + 1, ly.wo,
                                         sc.delta, sh.Hs, sh.Hkvs, D.d, D.h, (int64_t)c->seq_alloc, D.scale));
            } else if (c->rep_attn) {
                AttnRepArgs ra;
                ra.q = sc.q; ra.kc = kv.k; ra.vT = kv.v; ra.st = cs.st; ra.Wo = ly.wo; ra.out = sc.delta;
                ra.H = (int)sh.Hs; ra.Hkv = (int)sh.Hkvs; ra.seq_alloc = (int)c->seq_alloc; ra.N = (int)D.h; ra.K = (int)(sh.Hs * D.d); ra.scale = D.scale;
                if (far) { ra.ll = sh.pc.ll_dev; ra.ll_slot = (int)(2 * l + 1); }
                FL_TRY(launch_attn_oproj_rep(L, ra));
            } else {
                FL_TRY(attend_decode(L, m, c, sh, cs, kv, sc.q, sc.ao, as));
                o_done = edge_fits(sh.Hs * D.d, 2 * sh.Ip);
                if (o_done) FL_TRY(producer(L, sc, ly.wo, sc.ao, sh.Hs * D.d, sc.x_res2, sc.x_res, ly.ln2));
                else if (w8) FL_TRY(plain_w8(L, ly.wo8, ly.so, sc.ao, sh.Hs * D.d, sc.delta));
                else if (far) FL_TRY(row_parallel(L, sh, ly.wo, sc.ao, sh.Hs * D.d, sc.delta, (int)(2 * l + 1)));
                else FL_TRY(launch_linear(L, dt, ly.wo, sc.ao, nullptr, sc.delta, 1, D.h, sh.Hs * D.d, EPI_F32));
            }
            return FL_OK;
        }));
        if (!far) FL_TRY(all_reduce_delta(m, false, D.h));
        FL_TRY(each_shard(m, c, [&](Shard &sh, CacheShard &cs, Launcher &L) -> int {
            Scratch &sc = sh.dec; LayerW &ly = sh.layers[l];
            GemvArgs a;
            a.W = ly.wgu; a.out = sc.act; a.N = (int)(2 * sh.Ip); a.K = (int)D.h; a.epi = EPI_GATEUP; a.pro = PRO_NORM;
            a.x_in = sc.x_res2; a.delta = sc.delta; a.norm_w = ly.ln2; a.eps = D.eps; a.x_out = sc.x_res; a.st = cs.st;
            if (c->fuse_oproj) a.delta_nslab = (int)sh.Hkvs;           // one partial vector per kv head
            if (o_done) take_finished_norm(a, sc);
            FL_TRY(gemv(L, a, ly.wgu8, ly.sgu));
            const bool last = l + 1 == D.L;
            down_done = edge_fits(sh.Ip, last ? sh.Vs : (sh.Hs + 2 * sh.Hkvs) * D.d);
            if (down_done) FL_TRY(producer(L, sc, ly.wd, sc.act, sh.Ip, sc.x_res, sc.x_res2, last ? sh.norm : sh.layers[l + 1].ln1));
            else if (w8) FL_TRY(plain_w8(L, ly.wd8, ly.sd, sc.act, sh.Ip, sc.delta));
            else if (far) FL_TRY(row_parallel(L, sh, ly.wd, sc.act, sh.Ip, sc.delta, (int)(2 * l + 2)));
            else FL_TRY(launch_linear(L, dt, ly.wd, sc.act, nullptr, sc.delta, 1, D.h, sh.Ip, EPI_F32));
            return FL_OK;
        }));
        if (!far) FL_TRY(all_reduce_delta(m, false, D.h));
    }
    FL_TRY(each_shard(m, c, [&](Shard &sh, CacheShard &cs, Launcher &L) -> int {
        Scratch &sc = sh.dec;
        GemvArgs a;
        a.W = sh.lm_head; a.out = lm_head_out(m, sh); a.N = (int)sh.Vs; a.K = (int)D.h; a.epi = EPI_F32; a.pro = PRO_NORM;
        if (!m->vocab_parallel && tune(TK_ARGMAX_FUSED) && (w8 ? gemv_w8_leaves_candidates(a.N, a.K) : gemv_leaves_candidates(dt, a))) { a.amax = sh.amax; sh.amax_valid = true; }   // token selection reads one candidate per workgroup
        a.x_in = sc.x_res; a.delta = sc.delta; a.norm_w = sh.norm; a.eps = D.eps; a.st = cs.st;
        if (down_done) take_finished_norm(a, sc);
        return gemv(L, a, sh.lm_head8, sh.lm_head_s);
    }));
    return gather_logits(m);
}

// all-reduce(sum) of rows [off, off + count) floats of every local shard's prefill delta, on the shards' comm streams
static int all_reduce_span_side(Model *m, size_t off, int64_t count) {
    const bool local = m->tp_mode == FL_TP_SINGLE_PROCESS;
    Shard &s0 = m->shards[0];
    if (s0.pc.connected && (count <= s0.pc.nmax || !s0.comm)) {
        for (auto &sh : m->shards) {
            FL_HIP(hipSetDevice(sh.device));
            FL_TRY(oneshot(m, sh, false, sh.pre.delta + off, sh.pre.delta + off, count, 0, sh.comm_stream));
        }
        return FL_OK;
    }
    if (!s0.comm) FL_FAIL(FL_ERR_RCCL, "tensor-parallel group is not connected: call fl_comm_ipc_connect first");
    if (local) FL_NCCL(ncclGroupStart());
    for (auto &sh : m->shards)
        FL_NCCL(ncclAllReduce(sh.pre.delta + off, sh.pre.delta + off, (size_t)count, ncclFloat, ncclSum, sh.comm, sh.comm_stream));
    if (local) FL_NCCL(ncclGroupEnd());
    return FL_OK;
}

// narrow(1, T-1, 1) -> final norm -> lm_head on the last position only (K12).  norm_done: a residual epilogue has already left the
// row's xn and 1/rms; else the norm sums the nslab slabs of delta
static int last_row_logits(Launcher &L, Model *m, Shard &sh, Scratch &sc, int64_t T, bool norm_done, int nslab, int64_t slab) {
    const Dims &D = m->D;
    const size_t r = (size_t)(T - 1);
    void *xnl = (char *)sc.xn + r * D.h * m->esize();
    if (!norm_done) FL_TRY(launch_rmsnorm_add(L, m->dtype, sc.x_res + r * D.h, sc.delta + r * D.h, sh.norm, D.eps, xnl, sc.inv_rms + r, 1, D.h, nslab, slab));
    return launch_linear(L, m->dtype, sh.lm_head, xnl, nullptr, lm_head_out(m, sh), 1, sh.Vs, D.h, EPI_F32, sc.inv_rms + r);
}

// Tensor-parallel prefill with the all-reduces on a side stream (north_star: "RCCL all-reduce ... overlapped on a side
// HIP stream").  The T tokens are cut into two row chunks; every op between attention and the next attention is
// row-wise, so while chunk 0's o_proj output is being all-reduced, chunk 1's o_proj runs; while chunk 1's is reduced,
// chunk 0's norm / gate-up / down run; and so on into the next layer's norm + QKV.  Only RoPE / attention wait for both.
//   main:  ... attn(all) | o(c0) e0 | o(c1) e1 | wait h0: mlp(c0) f0 | wait h1: mlp(c1) f1 | wait g0: qkv(c0) | wait g1: qkv(c1) | rope, attn ...
//   comm:                 wait e0: AR(c0) h0 | wait e1: AR(c1) h1 | wait f0: AR(c0) g0 | wait f1: AR(c1) g1
static int enqueue_prefill_tp_overlap(Model *m, Cache *c, int64_t T) {
    const Dims &D = m->D;
    const int dt = m->dtype;
    const size_t es = m->esize();
    const int64_t T0 = std::min<int64_t>(T - 1, ((T / 2 + 255) / 256) * 256), T1 = T - T0;
    const int64_t rows[2] = {T0, T1}, row0[2] = {0, T0};
    enum { E0 = 0, E1, H0, H1, F0, F1, G0, G1 };
    FL_TRY(each_shard(m, c, [&](Shard &sh, CacheShard &cs, Launcher &L) -> int {
        if (!sh.comm_stream) FL_HIP(hipStreamCreateWithFlags(&sh.comm_stream, hipStreamNonBlocking));
        for (auto &e : sh.ev) if (!e) FL_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        return launch_embed(L, dt, sh.embed, sh.pre.ids, cs.st, sh.pre.x_res, T, D.h);
    }));
    auto rec = [&](int ev, bool side) { return each_shard(m, c, [&](Shard &sh, CacheShard &, Launcher &) -> int { FL_HIP(hipEventRecord(sh.ev[ev], side ? sh.comm_stream : sh.stream)); return FL_OK; }); };
    auto wait = [&](int ev, bool side) { return each_shard(m, c, [&](Shard &sh, CacheShard &, Launcher &) -> int { FL_HIP(hipStreamWaitEvent(side ? sh.comm_stream : sh.stream, sh.ev[ev], 0)); return FL_OK; }); };
    for (int64_t l = 0; l < D.L; l++) {
        for (int k = 0; k < 2; k++) {                                  // norm1 + QKV per chunk, as soon as its rows are reduced
            if (l > 0) FL_TRY(wait(G0 + k, false));
            FL_TRY(each_shard(m, c, [&](Shard &sh, CacheShard &, Launcher &L) -> int {
                Scratch &sc = sh.pre; LayerW &ly = sh.layers[l];
                const int64_t nq = (sh.Hs + 2 * sh.Hkvs) * D.d;
                const size_t r = (size_t)row0[k];
                FL_TRY(launch_rmsnorm_add(L, dt, sc.x_res + r * D.h, l == 0 ? nullptr : sc.delta + r * D.h, ly.ln1, D.eps, (char *)sc.xn + r * D.h * es,
                                          sc.inv_rms + r, rows[k], D.h, 1, 0));
                return launch_linear(L, dt, ly.wqkv, (char *)sc.xn + r * D.h * es, ly.bqkv, sc.qkv + r * nq, rows[k], nq, D.h, EPI_F32, sc.inv_rms + r);
            }));
        }
        FL_TRY(each_shard(m, c, [&](Shard &sh, CacheShard &cs, Launcher &L) -> int {
            Scratch &sc = sh.pre;
            const KvLayer kv(m, c, sh, cs, l);
            FL_TRY(launch_rope_kv(L, dt, sc.qkv, cs.st, sh.cos_tab, sh.sin_tab, D.max_pos, sc.q, kv.k, kv.v, T, sh.Hs, sh.Hkvs, D.d, (int64_t)c->seq_alloc, c->v_transposed));
            return attend_prefill(L, m, c, sh, cs, kv, sc, T);
        }));
        for (int k = 0; k < 2; k++) {                                  // o_proj per chunk; its all-reduce goes to the side stream
            FL_TRY(each_shard(m, c, [&](Shard &sh, CacheShard &, Launcher &L) -> int {
                Scratch &sc = sh.pre;
                const size_t r = (size_t)row0[k];
                return launch_linear(L, dt, sh.layers[l].wo, (char *)sc.ao + r * sh.Hs * D.d * es, nullptr, sc.delta + r * D.h, rows[k], D.h, sh.Hs * D.d, EPI_F32);
            }));
            FL_TRY(rec(E0 + k, false));
            FL_TRY(wait(E0 + k, true));
            FL_TRY(all_reduce_span_side(m, (size_t)row0[k] * D.h, rows[k] * D.h));
            FL_TRY(rec(H0 + k, true));
        }
        for (int k = 0; k < 2; k++) {                                  // MLP per chunk
            FL_TRY(wait(H0 + k, false));
            FL_TRY(each_shard(m, c, [&](Shard &sh, CacheShard &, Launcher &L) -> int {
                Scratch &sc = sh.pre; LayerW &ly = sh.layers[l];
                const size_t r = (size_t)row0[k];
                FL_TRY(launch_rmsnorm_add(L, dt, sc.x_res + r * D.h, sc.delta + r * D.h, ly.ln2, D.eps, (char *)sc.xn + r * D.h * es, sc.inv_rms + r, rows[k], D.h, 1, 0));
                FL_TRY(launch_linear(L, dt, ly.wgu, (char *)sc.xn + r * D.h * es, nullptr, (char *)sc.act + r * sh.Ip * es, rows[k], 2 * sh.Ip, D.h, EPI_GATEUP, sc.inv_rms + r));
                return launch_linear(L, dt, ly.wd, (char *)sc.act + r * sh.Ip * es, nullptr, sc.delta + r * D.h, rows[k], D.h, sh.Ip, EPI_F32);
            }));
            FL_TRY(rec(F0 + k, false));
            FL_TRY(wait(F0 + k, true));
            FL_TRY(all_reduce_span_side(m, (size_t)row0[k] * D.h, rows[k] * D.h));
            FL_TRY(rec(G0 + k, true));
        }
    }
    FL_TRY(wait(G1, false));                                           // the last token lives in chunk 1
    FL_TRY(each_shard(m, c, [&](Shard &sh, CacheShard &, Launcher &L) { return last_row_logits(L, m, sh, sh.pre, T, false, 1, 0); }));
    FL_TRY(wait(G0, false));                                           // nothing of this call may still run on the side stream afterwards
    return gather_logits(m);
}

ResidEpi resid_epi(const Scratch &sc, const Dims &D, const float *next_norm_w) {
    ResidEpi re;
    re.h = sc.x_res; re.w = next_norm_w; re.xn = sc.xn; re.part = sc.rs_part; re.np = gemm_resid_partials(D.h);
    return re;
}

// lm_head on the T rows whose xn and 1/rms the final norm has left in sc, in blocks of at most rows.R rows into rows.out; rows.each
// (if any) is enqueued behind every block, before the next one overwrites it
int lm_head_rows(Model *m, Shard &sh, Launcher &L, Scratch &sc, int64_t T, const AllRows &rows) {
    const Dims &D = m->D;
    for (int64_t r0 = 0, n = 0; r0 < T; r0 += n) {
        n = std::min<int64_t>(rows.R, T - r0);
        if (rows.no_one_row_tail && T - r0 - n == 1 && n > 2) n -= 1;
        FL_TRY(launch_linear(L, m->dtype, sh.lm_head, (char *)sc.xn + (size_t)r0 * D.h * m->esize(), nullptr, rows.out, n, sh.Vs, D.h, EPI_F32, sc.inv_rms + r0));
        if (rows.each) FL_TRY(rows.each(L, r0, n));
    }
    return FL_OK;
}

// Enqueue one forward over T tokens on every local shard.  The step state (pos, len, token) of the
// cache must already be set on the device.  ids_dev == null: the single token comes from the state.
// all_rows (a verify step or a scored forward, one shard): the final norm and lm_head run on EVERY row (lm_head_rows: in blocks of
// all_rows->R rows into all_rows->out, a verify step's one block being all of its rows), and the last row's logits are NOT left in
// logits_full; null: the last position only, exactly the launches there have always been.
static int enqueue_forward(Model *m, Cache *c, bool pre, int64_t T, bool ids_in_scratch, int64_t len_hint, const AllRows *all_rows = nullptr) {
    for (auto &sh : m->shards) sh.amax_valid = false;                  // (set by the path whose lm_head launch leaves ArgMax candidates)
    if (T == 1 && !pre && !ids_in_scratch && m->fused_decode) return enqueue_decode_fused(m, c, len_hint);
    if (pre && ids_in_scratch && m->tp > 1 && tune(TK_TP_OVERLAP) && T >= tune(TK_TP_OVERLAP_MIN_T) && !m->profiling &&
        (m->tp_mode == FL_TP_MULTI_PROCESS || m->tp_mode == FL_TP_SINGLE_PROCESS))
        return enqueue_prefill_tp_overlap(m, c, T);
    const Dims &D = m->D;
    const int dt = m->dtype;
    auto SC = [&](Shard &sh) -> Scratch & { return pre ? sh.pre : sh.dec; };
    FL_TRY(each_shard(m, c, [&](Shard &sh, CacheShard &cs, Launcher &L) {
        return launch_embed(L, dt, sh.embed, ids_in_scratch ? SC(sh).ids : nullptr, cs.st, SC(sh).x_res, T, D.h);
    }));
    // split-K of the row-parallel GEMMs (o_proj, down_proj) only without tensor parallelism: the
    // all-reduce wants one summed buffer
    const int max_split = (m->tp == 1 && T > 1) ? ksplit_cap(T) : 1;
    const int64_t slab = T * D.h;
    int nslab = 1;                        // slabs the current delta consists of (same on every shard)
    // Long prompts on one GPU: where the 256x256 kernel takes o_proj / down_proj in one piece, its epilogue adds the residual,
    // writes the next norm's x * w and leaves partial sums of squares (EPI_RESID) -- no delta round trip, no rmsnorm_add launch.
    const bool resid_ok = m->shards.size() == 1 && m->tp == 1 && !m->shards[0].comm && dt == FL_DTYPE_BF16 && T > 1 && SC(m->shards[0]).rs_part != nullptr;
    bool norm_done = false;               // xn / inv_rms for the upcoming norm were produced by the previous projection
    // consumer_takes_parts: the projection that follows takes its row scales (1/rms) straight from the partial sums (Launcher::rsp,
    // kernels.h) -- then there is no rms_finalize launch either; rs_lazy says so until that projection is launched
    bool rs_lazy = false;
    auto linear_resid = [&](Launcher &L, Scratch &sc, const LinearPlan &p, const void *W, const void *x, int64_t K, const float *next_norm_w,
                            bool consumer_takes_parts) -> int {
        const ResidEpi re = resid_epi(sc, D, next_norm_w);
        FL_TRY(launch_plan(L, p, dt, W, x, nullptr, nullptr, T, D.h, K, EPI_RESID, nullptr, &re));
        // (A/B, whole prefills: Mistral-7B 384 / 512 / 640 tokens 0.987 / 0.997 / 0.999, 4096 tokens 1.011: every workgroup of a long
        // prompt's grid sums 256 rows' partials again, the finalize launch does it once)
        rs_lazy = consumer_takes_parts && tune(TK_RS_LAZY) != 0 && T <= 1024;
        if (rs_lazy) return FL_OK;
        return launch_rms_finalize(L, sc.rs_part, re.np, D.eps, sc.inv_rms, T, D.h);
    };
    auto with_parts = [&](Launcher &L, Scratch &sc) {             // the launcher of the projection behind a lazy residual epilogue
        if (rs_lazy) { L.rsp = RsParts{sc.rs_part, gemm_resid_partials(D.h), D.eps, 1.0f / (float)D.h}; rs_lazy = false; }
    };
    for (int64_t l = 0; l < D.L; l++) {
        FL_TRY(each_shard(m, c, [&](Shard &sh, CacheShard &cs, Launcher &L) -> int {
            Scratch &sc = SC(sh); LayerW &ly = sh.layers[l];
            const int64_t nq = (sh.Hs + 2 * sh.Hkvs) * D.d;
            const KvLayer kv(m, c, sh, cs, l);
            if (!norm_done) FL_TRY(launch_rmsnorm_add(L, dt, sc.x_res, l == 0 ? nullptr : sc.delta, ly.ln1, D.eps, sc.xn, sc.inv_rms, T, D.h, nslab, slab));
            norm_done = false;
            // (Qwen2's q/k/v bias moves into the RoPE launch, which sums the slabs anyway: with the bias in the GEMM epilogue the
            // projection could not run in K slices and a mid-size prompt's QKV sat on 128x128 tiles -- T = 512: 63 us at 0.27 PFLOP/s)
            const int64_t sa = (int64_t)c->seq_alloc;
            with_parts(L, sc);                                       // (the previous layer's down_proj may have left 1/rms as partial sums)
            const LinearPlan qp = plan_qkv_rope(dt, T, nq, D.h, D.d, D.d * sh.Hkvs, m->tp, qkv_split(T));
            if (qp.rope) {
                // RoPE, bias and the KV append ride in the projection's epilogue: no fp32 QKV matrix
                RopeEpi ro;
                ro.st = cs.st; ro.cos_tab = sh.cos_tab; ro.sin_tab = sh.sin_tab; ro.max_pos = (int)D.max_pos; ro.q_out = sc.q; ro.k_cache = kv.k; ro.v_cache = kv.v;
                ro.H = (int)sh.Hs; ro.Hkv = (int)sh.Hkvs; ro.d = (int)D.d; ro.max_seq = (int)sa; ro.v_transposed = c->v_transposed ? 1 : 0;
                FL_TRY(launch_plan(L, qp, dt, ly.wqkv, sc.xn, ly.bqkv, nullptr, T, nq, D.h, EPI_QKV_ROPE, sc.inv_rms, nullptr, &ro));
            } else {
                FL_TRY(launch_plan(L, qp, dt, ly.wqkv, sc.xn, nullptr, sc.qkv, T, nq, D.h, EPI_F32, sc.inv_rms));
                FL_TRY(launch_rope_kv(L, dt, sc.qkv, cs.st, sh.cos_tab, sh.sin_tab, D.max_pos, sc.q, kv.k, kv.v, T, sh.Hs, sh.Hkvs, D.d, sa, c->v_transposed, qp.n_split, ly.bqkv));
            }
            L.rsp = RsParts{};
            if (T == 1) {
                const AttnScratch as{cs.part_m, cs.part_l, cs.part_o, cs.counters, c->nsplit, len_hint + 1};
                FL_TRY(attend_decode(L, m, c, sh, cs, kv, sc.q, sc.ao, as));
            } else {
                FL_TRY(attend_prefill(L, m, c, sh, cs, kv, sc, T));
            }
            const LinearPlan op = resid_ok ? plan_resid(dt, T, D.h, sh.Hs * D.d, max_split, false) : LinearPlan{};
            if (op.kernel != LK_NONE) {
                const bool gu_parts = plan_linear(dt, T, 2 * sh.Ip, D.h, EPI_GATEUP, m->tp, 1, false, false, false).reads_rs_parts;
                FL_TRY(linear_resid(L, sc, op, ly.wo, sc.ao, sh.Hs * D.d, ly.ln2, gu_parts));
                norm_done = true;
            } else {
                FL_TRY(launch_linear(L, dt, ly.wo, sc.ao, nullptr, sc.delta, T, D.h, sh.Hs * D.d, EPI_F32, nullptr, max_split, &nslab));
            }
            return FL_OK;
        }));
        FL_TRY(all_reduce_delta(m, pre, T * D.h));
        FL_TRY(each_shard(m, c, [&](Shard &sh, CacheShard &, Launcher &L) -> int {
            Scratch &sc = SC(sh); LayerW &ly = sh.layers[l];
            if (!norm_done) FL_TRY(launch_rmsnorm_add(L, dt, sc.x_res, sc.delta, ly.ln2, D.eps, sc.xn, sc.inv_rms, T, D.h, nslab, slab));
            norm_done = false;
            with_parts(L, sc);
            FL_TRY(launch_linear(L, dt, ly.wgu, sc.xn, nullptr, sc.act, T, 2 * sh.Ip, D.h, EPI_GATEUP, sc.inv_rms));
            L.rsp = RsParts{};
            const LinearPlan dp = resid_ok ? plan_resid(dt, T, D.h, sh.Ip, max_split, false) : LinearPlan{};
            if (dp.kernel != LK_NONE) {
                // (the next layer's QKV projection takes the partial sums if its kernel can; the last layer's final norm wants the vector)
                const int64_t nq = (sh.Hs + 2 * sh.Hkvs) * D.d;
                const bool qkv_parts = l + 1 < D.L && plan_qkv_rope(dt, T, nq, D.h, D.d, D.d * sh.Hkvs, m->tp, qkv_split(T)).reads_rs_parts;
                FL_TRY(linear_resid(L, sc, dp, ly.wd, sc.act, sh.Ip, l + 1 < D.L ? sh.layers[l + 1].ln1 : sh.norm, qkv_parts));
                norm_done = true;
            } else {
                FL_TRY(launch_linear(L, dt, ly.wd, sc.act, nullptr, sc.delta, T, D.h, sh.Ip, EPI_F32, nullptr, max_split, &nslab));
            }
            return FL_OK;
        }));
        FL_TRY(all_reduce_delta(m, pre, T * D.h));
    }
    if (all_rows) {
        // every row: the residual epilogue of the last down_proj has left xn and 1/rms of all T rows (norm_done; the last layer's is
        // always finalized to the vector), or rmsnorm_add produces them here
        Shard &sh = m->shards[0]; Scratch &sc = SC(sh);
        FL_HIP(hipSetDevice(sh.device));
        Launcher L = make_launcher(m, sh);
        if (!norm_done) FL_TRY(launch_rmsnorm_add(L, dt, sc.x_res, sc.delta, sh.norm, D.eps, sc.xn, sc.inv_rms, T, D.h, nslab, slab));
        return lm_head_rows(m, sh, L, sc, T, *all_rows);
    }
    FL_TRY(each_shard(m, c, [&](Shard &sh, CacheShard &, Launcher &L) { return last_row_logits(L, m, sh, SC(sh), T, norm_done, nslab, slab); }));
    return gather_logits(m);
}

// sampler: non-null (re)sets the cache's token selection; null keeps it (later chunks of one call)
static int set_state(Model *m, Cache *c, uint32_t token, size_t pos, size_t len, uint32_t step, int64_t eos, size_t call0 = (size_t)-1,
                     const SampleState *sampler = nullptr) {
    if (call0 == (size_t)-1) call0 = len;
    return each_shard(m, c, [&](Shard &sh, CacheShard &cs, Launcher &) {
        return set_shard_state(m, sh, cs, token, pos, len, call0, step, eos, sampler ? *sampler : SampleState{}, sampler != nullptr);
    });
}

// rules: the cache's logit rules are on -- logit_rules_kernel leaves the adjusted row in logits_adj, and the selection reads that, as
// a full pass (the lm_head epilogue's ArgMax candidates belong to the raw row); off: exactly the launch there has always been
// guide: a guide is installed too -- guide_mask_kernel then leaves that row (or the raw one) masked in logits_guided, the last word
static int enqueue_argmax(Model *m, Cache *c, int advance, bool rules = false, bool guide = false) {
    return each_shard(m, c, [&](Shard &sh, CacheShard &cs, Launcher &L) -> int {
        if (rules || guide) {
            const float *row = sh.logits_full;
            if (rules) {
                LogitRulesSrc src;
                src.st = cs.st; src.ctl = cs.rule_ctl;
                FL_TRY(launch_logit_rules(L, row, m->D.V, 1, src));
                row = cs.logits_adj;
            }
            if (guide) {
                GuideSrc src;
                src.st = cs.st; src.ctl = cs.guide_ctl;
                FL_TRY(launch_guide_mask(L, row, m->D.V, 1, src));
                row = cs.logits_guided;
            }
            return launch_select_advance(L, row, m->D.V, cs.st, cs.ss, cs.sel_scratch, cs.out_tokens, advance, nullptr, sh.eng_epoch);
        }
        return launch_select_advance(L, sh.logits_full, m->D.V, cs.st, cs.ss, cs.sel_scratch, cs.out_tokens, advance, sh.amax_valid ? sh.amax : nullptr, sh.eng_epoch);
    });
}

// ---- logit rules (fl_cache_set_logit_rules)
int check_logit_rules(const fl_logit_rules *r, const uint32_t *prompt_ids, size_t n_prompt, const uint32_t *output_ids, size_t n_output, int64_t V) {
    if (!r) FL_FAIL(FL_ERR_BAD_ARGUMENT, "null fl_logit_rules (rules)");
    if (r->struct_size != sizeof(fl_logit_rules)) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_logit_rules.struct_size is %u, expected %zu", r->struct_size, sizeof(fl_logit_rules));
    if (r->_reserved[0] || r->_reserved[1]) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_logit_rules._reserved must be 0");
    if (!isfinite(r->repetition_penalty) || !(r->repetition_penalty > 0.f)) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_logit_rules.repetition_penalty must be finite and > 0");
    if (!isfinite(r->frequency_penalty)) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_logit_rules.frequency_penalty must be finite");
    if (!isfinite(r->presence_penalty)) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_logit_rules.presence_penalty must be finite");
    if (r->n_bias && (!r->bias_ids || !r->bias_values)) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_logit_rules.bias_ids / bias_values is null with n_bias %u", r->n_bias);
    if (n_prompt && !prompt_ids) FL_FAIL(FL_ERR_BAD_ARGUMENT, "null prompt_ids with n_prompt %zu", n_prompt);
    if (n_output && !output_ids) FL_FAIL(FL_ERR_BAD_ARGUMENT, "null output_ids with n_output %zu", n_output);
    for (uint32_t i = 0; i < r->n_bias; i++) {
        const float v = r->bias_values[i];
        if (v != v || v == INFINITY) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_logit_rules.bias_values[%u] is NaN or +inf", i);
    }
    if (V > 0) {
        if ((int64_t)r->n_bias > V) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_logit_rules.n_bias %u exceeds the vocabulary %lld", r->n_bias, (long long)V);
        for (uint32_t i = 0; i < r->n_bias; i++)
            if ((int64_t)r->bias_ids[i] >= V) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_logit_rules.bias_ids[%u] = %u out of range (vocab %lld)", i, r->bias_ids[i], (long long)V);
        for (size_t i = 0; i < n_prompt; i++)
            if ((int64_t)prompt_ids[i] >= V) FL_FAIL(FL_ERR_BAD_ARGUMENT, "prompt_ids[%zu] = %u out of range (vocab %lld)", i, prompt_ids[i], (long long)V);
        for (size_t i = 0; i < n_output; i++)
            if ((int64_t)output_ids[i] >= V) FL_FAIL(FL_ERR_BAD_ARGUMENT, "output_ids[%zu] = %u out of range (vocab %lld)", i, output_ids[i], (long long)V);
    }
    std::vector<uint32_t> sorted(r->bias_ids, r->bias_ids + r->n_bias);
    std::sort(sorted.begin(), sorted.end());
    for (size_t i = 1; i < sorted.size(); i++)
        if (sorted[i] == sorted[i - 1]) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_logit_rules.bias_ids: duplicate id %u", sorted[i]);
    return FL_OK;
}

int refuse_logit_rules(const Cache *c, const char *what) {
    if (c && c->rules_on) FL_FAIL(FL_ERR_UNSUPPORTED, "%s does not honour logit rules: remove them from the cache first (fl_cache_set_logit_rules with NULL)", what);
    return FL_OK;
}

int cache_set_logit_rules(Model *m, Cache *c, const fl_logit_rules *rules, const uint32_t *prompt_ids, size_t n_prompt, const uint32_t *output_ids, size_t n_output) {
    if (rules) FL_TRY(check_logit_rules(rules, prompt_ids, n_prompt, output_ids, n_output, 0));
    if (!m || !c) FL_FAIL(FL_ERR_BAD_ARGUMENT, "null model or cache");
    if (c->m != m) FL_FAIL(FL_ERR_BAD_ARGUMENT, "cache belongs to another model");
    if (!rules) {                                                     // removal: the buffers stay (freed with the cache), the old graphs run again
        std::lock_guard<std::mutex> lock(m->mu);
        c->rules_on = false;
        return FL_OK;
    }
    const int64_t V = m->D.V;
    FL_TRY(check_logit_rules(rules, prompt_ids, n_prompt, output_ids, n_output, V));
    if (m->tp > 1 || m->shards.size() != 1) FL_FAIL(FL_ERR_UNSUPPORTED, "logit rules do not run under tensor parallelism (tp_size %d)", m->tp);
    if (n_output > 0x7fffffffu) FL_FAIL(FL_ERR_BAD_ARGUMENT, "n_output %zu exceeds the 31-bit count", n_output);
    std::lock_guard<std::mutex> lock(m->mu);
    Shard &sh = m->shards[0]; CacheShard &cs = c->shards[0];
    FL_HIP(hipSetDevice(sh.device));
    if (!cs.rule_image) FL_HIP(hipHostMalloc((void **)&cs.rule_image, (size_t)V * sizeof(LogitRuleEntry), hipHostMallocDefault));
    else FL_HIP(hipStreamSynchronize(sh.stream));                     // (the previous install's copy reads the image)
    if (!cs.rule_tab) FL_TRY(dev_alloc(cs.allocs, (void **)&cs.rule_tab, (size_t)V * sizeof(LogitRuleEntry), nullptr));
    if (!cs.rule_ctl) FL_TRY(dev_alloc(cs.allocs, (void **)&cs.rule_ctl, sizeof(LogitRulesCtl), nullptr));
    if (!cs.logits_adj) FL_TRY(dev_alloc(cs.allocs, (void **)&cs.logits_adj, (size_t)V * 4, nullptr));
    LogitRuleEntry *img = cs.rule_image;
    for (int64_t j = 0; j < V; j++) img[j] = LogitRuleEntry{0u, 0.f};
    for (size_t i = 0; i < n_prompt; i++) img[prompt_ids[i]].word |= kRulePromptBit;
    for (size_t i = 0; i < n_output; i++) img[output_ids[i]].word += 1;          // (n_output < 2^31: no carry into the prompt bit)
    for (uint32_t i = 0; i < rules->n_bias; i++) img[rules->bias_ids[i]].bias = rules->bias_values[i];
    FL_HIP(hipMemcpyAsync(cs.rule_tab, img, (size_t)V * sizeof(LogitRuleEntry), hipMemcpyHostToDevice, sh.stream));
    c->rule_rp = rules->repetition_penalty; c->rule_fp = rules->frequency_penalty; c->rule_pp = rules->presence_penalty;
    c->rules_on = true;
    return FL_OK;
}

int cache_logit_counts(Model *m, Cache *c, uint32_t *words_out) {
    if (!m || !c || !words_out) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_cache_logit_counts: null argument");
    if (c->m != m) FL_FAIL(FL_ERR_BAD_ARGUMENT, "cache belongs to another model");
    if (!c->rules_on) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_cache_logit_counts: the cache has no logit rules installed");
    std::lock_guard<std::mutex> lock(m->mu);
    Shard &sh = m->shards[0]; CacheShard &cs = c->shards[0];
    FL_HIP(hipSetDevice(sh.device));
    FL_HIP(hipStreamSynchronize(sh.stream));
    std::vector<LogitRuleEntry> tab((size_t)m->D.V);
    FL_HIP(hipMemcpy(tab.data(), cs.rule_tab, tab.size() * sizeof(LogitRuleEntry), hipMemcpyDeviceToHost));
    for (size_t j = 0; j < tab.size(); j++) words_out[j] = tab[j].word;
    return FL_OK;
}

int set_logit_rules_ctl(Model *m, Cache *c, bool count_input) {
    Shard &sh = m->shards[0]; CacheShard &cs = c->shards[0];
    Launcher L = make_launcher(m, sh);
    return launch_set_logit_rules_ctl(L, cs.rule_ctl, LogitRulesCtl{c->rule_rp, c->rule_fp, c->rule_pp, count_input ? 1u : 0u, cs.rule_tab, cs.logits_adj});
}

// ---- guided decoding (fl_guide_create, fl_cache_set_guide)
int check_guide(const fl_guide_desc *d, int64_t V) {
    if (!d) FL_FAIL(FL_ERR_BAD_ARGUMENT, "null fl_guide_desc (desc)");
    if (d->struct_size != sizeof(fl_guide_desc)) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_guide_desc.struct_size is %u, expected %zu", d->struct_size, sizeof(fl_guide_desc));
    if (d->_reserved[0] || d->_reserved[1]) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_guide_desc._reserved must be 0");
    if (d->n_states == 0) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_guide_desc.n_states is 0");
    if (!d->row_ptr || !d->tokens || !d->next) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_guide_desc.row_ptr / tokens / next is null");
    if (d->row_ptr[0] != 0) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_guide_desc.row_ptr[0] is %llu, not 0", (unsigned long long)d->row_ptr[0]);
    for (uint32_t s = 0; s < d->n_states; s++) {                      // row_ptr as a whole first: it says how long the other two are
        const uint64_t r0 = d->row_ptr[s], r1 = d->row_ptr[s + 1];
        if (r1 < r0) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_guide_desc.row_ptr decreases at state %u", s);
        if (r1 == r0) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_guide_desc: state %u has no edge (every logit would be -inf)", s);
        if (r1 - r0 > 0x7fffffffull) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_guide_desc.row_ptr: state %u has more than 2^31 - 1 edges", s);
    }
    for (uint32_t s = 0; s < d->n_states; s++) {
        const uint64_t r0 = d->row_ptr[s], r1 = d->row_ptr[s + 1];
        for (uint64_t e = r0; e < r1; e++) {
            if (e > r0 && d->tokens[e] <= d->tokens[e - 1])
                FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_guide_desc.tokens of state %u are not strictly ascending (%u after %u)", s, d->tokens[e], d->tokens[e - 1]);
            if (V > 0 && (int64_t)d->tokens[e] >= V) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_guide_desc.tokens: id %u of state %u out of range (vocab %lld)", d->tokens[e], s, (long long)V);
            if (d->next[e] >= d->n_states) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_guide_desc.next: %u of state %u is not below n_states %u", d->next[e], s, d->n_states);
        }
    }
    return FL_OK;
}

uint32_t Guide::walk(uint32_t s, uint32_t t) const {
    const uint32_t *b = tokens.data() + row_ptr[s], *e = tokens.data() + row_ptr[s + 1];
    const uint32_t *it = std::lower_bound(b, e, t);
    return it != e && *it == t ? next[(size_t)(it - tokens.data())] : s;
}

Guide::~Guide() {
    if (!m) return;
    {
        std::lock_guard<std::mutex> lock(m->mu);
        (void)hipSetDevice(m->shards[0].device);
        (void)hipStreamSynchronize(m->shards[0].stream);
        if (row_ptr_dev) (void)hipFree(row_ptr_dev);
        if (tokens_dev) (void)hipFree(tokens_dev);
        if (next_dev) (void)hipFree(next_dev);
    }
    if (m->refs.fetch_sub(1) == 1) delete m;
}

void guide_release(Guide *g) {
    if (g && g->refs.fetch_sub(1) == 1) delete g;
}

int guide_create(Model *m, const fl_guide_desc *desc, Guide **out) {
    if (!out) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_guide_create: null out");
    *out = nullptr;
    FL_TRY(check_guide(desc, 0));
    if (!m) FL_FAIL(FL_ERR_BAD_ARGUMENT, "null model");
    FL_TRY(check_guide(desc, m->D.V));
    if (m->tp > 1 || m->shards.size() != 1) FL_FAIL(FL_ERR_UNSUPPORTED, "guided decoding does not run under tensor parallelism (tp_size %d)", m->tp);
    const size_t ns = desc->n_states, nnz = (size_t)desc->row_ptr[ns];
    std::unique_ptr<Guide> g(new Guide);
    g->n_states = desc->n_states;
    g->row_ptr.assign(desc->row_ptr, desc->row_ptr + ns + 1);
    g->tokens.assign(desc->tokens, desc->tokens + nnz);
    g->next.assign(desc->next, desc->next + nnz);
    {
        std::lock_guard<std::mutex> lock(m->mu);
        Shard &sh = m->shards[0];
        FL_HIP(hipSetDevice(sh.device));
        void *rp = nullptr, *tk = nullptr, *nx = nullptr;
        hipError_t e = hipMalloc(&rp, (ns + 1) * 8);
        if (e == hipSuccess) e = hipMalloc(&tk, nnz * 4);
        if (e == hipSuccess) e = hipMalloc(&nx, nnz * 4);
        if (e == hipSuccess) e = hipMemcpy(rp, g->row_ptr.data(), (ns + 1) * 8, hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(tk, g->tokens.data(), nnz * 4, hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(nx, g->next.data(), nnz * 4, hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            if (rp) (void)hipFree(rp);
            if (tk) (void)hipFree(tk);
            if (nx) (void)hipFree(nx);
            FL_FAIL(e == hipErrorOutOfMemory ? FL_ERR_OOM : FL_ERR_HIP, "fl_guide_create: %s (%zu states, %zu edges)", hipGetErrorString(e), ns, nnz);
        }
        g->row_ptr_dev = (uint64_t *)rp; g->tokens_dev = (uint32_t *)tk; g->next_dev = (uint32_t *)nx;
    }
    g->m = m;                                                         // (from here ~Guide frees the device copy and drops the model reference)
    m->refs.fetch_add(1);
    *out = g.release();
    return FL_OK;
}

int refuse_guide(const Cache *c, const char *what) {
    if (c && c->guide) FL_FAIL(FL_ERR_UNSUPPORTED, "%s does not honour a guide: remove it from the cache first (fl_cache_set_guide with NULL)", what);
    return FL_OK;
}

int cache_set_guide(Model *m, Cache *c, Guide *g, uint32_t state) {
    if (!m || !c) FL_FAIL(FL_ERR_BAD_ARGUMENT, "null model or cache");
    if (c->m != m) FL_FAIL(FL_ERR_BAD_ARGUMENT, "cache belongs to another model");
    Guide *old = nullptr;
    if (!g) {                                                         // removal: the buffers stay (freed with the cache), the old graphs run again
        std::lock_guard<std::mutex> lock(m->mu);
        old = c->guide;
        c->guide = nullptr;
    } else {
        if (g->m != m) FL_FAIL(FL_ERR_BAD_ARGUMENT, "the guide belongs to another model");
        if (state >= g->n_states) FL_FAIL(FL_ERR_BAD_ARGUMENT, "state %u is not below the guide's n_states %u", state, g->n_states);
        if (m->tp > 1 || m->shards.size() != 1) FL_FAIL(FL_ERR_UNSUPPORTED, "guided decoding does not run under tensor parallelism (tp_size %d)", m->tp);
        std::lock_guard<std::mutex> lock(m->mu);
        Shard &sh = m->shards[0]; CacheShard &cs = c->shards[0];
        FL_HIP(hipSetDevice(sh.device));
        if (!cs.guide_ctl) FL_TRY(dev_alloc(cs.allocs, (void **)&cs.guide_ctl, sizeof(GuideCtl), nullptr));
        if (!cs.logits_guided) FL_TRY(dev_alloc(cs.allocs, (void **)&cs.logits_guided, (size_t)m->D.V * 4, nullptr));
        if (c->guide != g) { old = c->guide; g->refs.fetch_add(1); c->guide = g; }
        c->guide_state = state;
    }
    if (old) guide_release(old);                                      // (outside the lock: the last reference frees under it)
    return FL_OK;
}

int cache_guide_state(const Cache *c, uint32_t *state_out) {
    if (!c || !state_out) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_cache_guide_state: null argument");
    if (!c->guide) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_cache_guide_state: the cache has no guide installed");
    *state_out = c->guide_state;
    return FL_OK;
}

int set_guide_ctl(Model *m, Cache *c) {
    Shard &sh = m->shards[0]; CacheShard &cs = c->shards[0];
    const Guide *g = c->guide;
    Launcher L = make_launcher(m, sh);
    return launch_set_guide_ctl(L, cs.guide_ctl, GuideCtl{g->row_ptr_dev, g->tokens_dev, g->next_dev, cs.logits_guided, {c->guide_state, c->guide_state}});
}

// ---- token log-probabilities (fl_*_lp)
int check_logprobs(const fl_logprobs *lp, int64_t V) {
    if (!lp) FL_FAIL(FL_ERR_BAD_ARGUMENT, "null fl_logprobs (lp)");
    if (lp->struct_size != sizeof(fl_logprobs)) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_logprobs.struct_size is %u, expected %zu", lp->struct_size, sizeof(fl_logprobs));
    if (lp->top_n < 0 || lp->top_n > FL_LOGPROBS_MAX_TOP) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_logprobs.top_n %d not in 0..%d", lp->top_n, FL_LOGPROBS_MAX_TOP);
    if (!lp->token_logprob) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_logprobs.token_logprob is null");
    if (lp->top_n > 0 && !lp->top_ids) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_logprobs.top_ids is null with top_n %d", lp->top_n);
    if (lp->top_n > 0 && !lp->top_logprobs) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_logprobs.top_logprobs is null with top_n %d", lp->top_n);
    if (lp->_reserved[0] || lp->_reserved[1]) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_logprobs._reserved must be 0");
    if (V > 0 && lp->top_n > V) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_logprobs.top_n %d exceeds the vocabulary %lld", lp->top_n, (long long)V);
    return FL_OK;
}

int logprobs_supported(const Model *m) {
    if (m->tp > 1 || m->shards.size() != 1) FL_FAIL(FL_ERR_UNSUPPORTED, "token log-probabilities do not run under tensor parallelism (tp_size %d)", m->tp);
    return FL_OK;
}

// the cache's record buffer and the model's pinned one, at the first call that asks (never inside a stream capture: the model is
// locked, and captures begin and end under that lock)
int ensure_logprobs(Model *m, Cache *c) {
    Shard &sh = m->shards[0]; CacheShard &cs = c->shards[0];
    FL_HIP(hipSetDevice(sh.device));
    if (!m->host_lp) FL_HIP(hipHostMalloc((void **)&m->host_lp, kOutTokensCap * sizeof(LogprobRec), hipHostMallocDefault));
    if (!cs.lp_recs) FL_TRY(dev_alloc(cs.allocs, (void **)&cs.lp_recs, kOutTokensCap * sizeof(LogprobRec), nullptr));
    if (!cs.lp_ctl) FL_TRY(dev_alloc(cs.allocs, (void **)&cs.lp_ctl, sizeof(LogprobCtl), nullptr));
    return FL_OK;
}

void scatter_logprobs(const LogprobRec &r, const fl_logprobs *lp, size_t at) {
    lp->token_logprob[at] = r.chosen;
    for (int j = 0; j < lp->top_n; j++) {
        lp->top_ids[at * (size_t)lp->top_n + (size_t)j] = r.ids[j];
        lp->top_logprobs[at * (size_t)lp->top_n + (size_t)j] = r.lps[j];
    }
}

// this call's top_n and record buffer, on the stream ahead of its steps
static int set_logprobs(Model *m, Cache *c, const fl_logprobs *lp) {
    Shard &sh = m->shards[0]; CacheShard &cs = c->shards[0];
    Launcher L = make_launcher(m, sh);
    return launch_set_logprob_ctl(L, cs.lp_ctl, cs.lp_recs, (uint32_t)kOutTokensCap, lp->top_n);
}

// right behind enqueue_argmax on the same stream: record `step - advance` of the cache
static int enqueue_logprobs(Model *m, Cache *c, int advance) {
    Shard &sh = m->shards[0]; CacheShard &cs = c->shards[0];
    Launcher L = make_launcher(m, sh);
    LogprobSrc src;
    src.st = cs.st; src.ctl = cs.lp_ctl;
    return launch_token_logprobs(L, sh.logits_full, m->D.V, 1, src, advance);
}

// The end of a call: n_tokens of the cache's token buffer and its StepState come back through the pinned buffers, every shard's
// stream is waited for, and the error word of the device-side waits and of the collectives is looked at.  n_lp: as many log-prob records too.
static int finish_call(Model *m, Cache *c, size_t n_tokens, size_t n_lp = 0) {
    Shard &s0 = m->shards[0];
    FL_HIP(hipSetDevice(s0.device));
    if (n_tokens) FL_HIP(hipMemcpyAsync(m->host_tokens, c->shards[0].out_tokens, n_tokens * 4, hipMemcpyDeviceToHost, s0.stream));
    if (n_lp) FL_HIP(hipMemcpyAsync(m->host_lp, c->shards[0].lp_recs, n_lp * sizeof(LogprobRec), hipMemcpyDeviceToHost, s0.stream));
    FL_HIP(hipMemcpyAsync(m->host_state, c->shards[0].st, sizeof(StepState), hipMemcpyDeviceToHost, s0.stream));
    FL_TRY(each_shard(m, c, [](Shard &sh, CacheShard &, Launcher &) -> int { FL_HIP(hipStreamSynchronize(sh.stream)); return FL_OK; }));
    if (m->host_state->error) FL_FAIL(FL_ERR_HIP, "device-side wait gave up (code 0x%x): decode kernels did not make progress", m->host_state->error);
    return comm_check(m);
}

int replay_or_capture(const std::vector<GraphSlot> &slots, bool graphable, bool &graph_failed, int &warm_steps, const std::function<int()> &enqueue) {
    auto launch_all = [&]() -> int {
        for (auto &s : slots) { FL_HIP(hipSetDevice(s.device)); FL_HIP(hipGraphLaunch(*s.exec, s.stream)); }
        return FL_OK;
    };
    if (graphable && *slots[0].exec) return launch_all();
    if (graphable && warm_steps >= 1) {
        const size_t ns = slots.size();
        std::vector<hipGraph_t> gs(ns, nullptr);
        bool ok = true;
        size_t begun = 0;
        for (; begun < ns; begun++) {
            FL_HIP(hipSetDevice(slots[begun].device));
            if (!(ok = hipStreamBeginCapture(slots[begun].stream, hipStreamCaptureModeThreadLocal) == hipSuccess)) break;
        }
        const int rc = ok ? enqueue() : FL_OK;
        for (size_t i = 0; i < begun; i++) {
            (void)hipSetDevice(slots[i].device);
            const hipError_t e = hipStreamEndCapture(slots[i].stream, &gs[i]);
            ok = ok && rc == FL_OK && e == hipSuccess && gs[i] != nullptr;
        }
        for (size_t i = 0; i < ns && ok; i++) {
            (void)hipSetDevice(slots[i].device);
            ok = hipGraphInstantiate(slots[i].exec, gs[i], nullptr, nullptr, 0) == hipSuccess;
        }
        for (auto g : gs) if (g) (void)hipGraphDestroy(g);
        if (ok) return launch_all();
        (void)hipGetLastError();
        for (auto &s : slots) if (*s.exec) { (void)hipGraphExecDestroy(*s.exec); *s.exec = nullptr; }
        graph_failed = true;                                        // fall through to eager launches
    }
    FL_TRY(enqueue());
    warm_steps++;
    return FL_OK;
}

// One decode step (embed .. lm_head .. argmax+advance) reading everything from the device state.
// Single-shard models replay it as a hipGraph (the ~11 launches per layer are launch-bound at
// TinyLlama scale); captured lazily on the second step of a cache so that all lazy module /
// attribute initialisation has already happened eagerly.
// kind (kStepLp | kStepRules | kStepGuide): the step with the log-prob launch behind token selection and / or the logit-rules and
// guide launches in front of it -- a graph of its own per kind; graph[0] is what it always was, and a cache may alternate between the kinds of call.
static int decode_step(Model *m, Cache *c, int64_t len_hint, int kind = 0) {
    // Graphs: one shard per process (plain single GPU, or one rank of a multi-process TP group: RCCL collectives are
    // stream-ordered and capturable, every rank captures the same sequence); or all shards of a single-process group
    // whose collectives are one-shot (they synchronise through memory, so each shard's step is its own graph).
    const int tp_graph = tune(TK_TP_GRAPH);
    const size_t ns = m->shards.size();
    const bool one_shard = ns == 1 && (m->tp == 1 || (m->tp_mode == FL_TP_MULTI_PROCESS && tp_graph));
    const bool local_group = ns > 1 && m->tp_mode == FL_TP_SINGLE_PROCESS && tp_graph && m->shards[0].pc.connected &&
                             m->D.h <= m->shards[0].pc.nmax && m->shards[0].Vs <= m->shards[0].pc.nmax;
    const bool graphable = m->use_graph && !m->profiling && (one_shard || local_group) && !c->graph_failed;
    std::vector<GraphSlot> slots;
    for (size_t i = 0; i < ns && graphable; i++)
        slots.push_back({m->shards[i].device, m->shards[i].stream, &c->shards[i].graph[kind]});
    return replay_or_capture(slots, graphable, c->graph_failed, c->warm_steps[kind], [&]() -> int {
        FL_TRY(enqueue_forward(m, c, false, 1, false, len_hint));
        FL_TRY(enqueue_argmax(m, c, 1, (kind & kStepRules) != 0, (kind & kStepGuide) != 0));
        return (kind & kStepLp) ? enqueue_logprobs(m, c, 1) : FL_OK;
    });
}

int check_call(Model *m, Cache *c, size_t T, size_t pos) {
    if (!m || !c) FL_FAIL(FL_ERR_BAD_ARGUMENT, "null model or cache");
    if (c->m != m) FL_FAIL(FL_ERR_BAD_ARGUMENT, "cache belongs to another model");
    if (T == 0) FL_FAIL(FL_ERR_BAD_ARGUMENT, "empty input");
    if (c->len + T > c->max_seq) FL_FAIL(FL_ERR_SEQ_OVERFLOW, "sequence overflow: %zu cached + %zu new > capacity %zu", c->len, T, c->max_seq);
    if (pos + T > (size_t)m->D.max_pos) FL_FAIL(FL_ERR_SEQ_OVERFLOW, "position %zu exceeds max_position_embeddings %lld", pos + T, (long long)m->D.max_pos);
    return FL_OK;
}

int check_token(const Model *m, uint32_t id, const char *what) {
    if ((int64_t)id >= m->D.V) FL_FAIL(FL_ERR_BAD_ARGUMENT, "%s id %u out of range (vocab %lld)", what, id, (long long)m->D.V);
    return FL_OK;
}

int forward(Model *m, Cache *c, const uint32_t *ids, size_t T, size_t pos, float *logits_out, uint32_t *token_out,
            const fl_sampler *sampling, const fl_logprobs *lp) {
    FL_TRY(check_call(m, c, T, pos));
    debug_inject("forward");
    SampleState sampler;
    FL_TRY(make_sampler(sampling, m->D.V, &sampler));
    if (!ids) FL_FAIL(FL_ERR_BAD_ARGUMENT, "null ids");
    for (size_t t = 0; t < T; t++) FL_TRY(check_token(m, ids[t], "token"));
    if (lp) { FL_TRY(check_logprobs(lp, m->D.V)); FL_TRY(logprobs_supported(m)); }
    std::lock_guard<std::mutex> lock(m->mu);
    if (lp) { FL_TRY(ensure_logprobs(m, c)); FL_TRY(set_logprobs(m, c, lp)); }
    const bool rules = c->rules_on;                  // (a forward's ids are prompt: the rules are applied, nothing is counted)
    if (rules) FL_TRY(set_logit_rules_ctl(m, c, false));
    const bool guide = c->guide && token_out;        // (fl_forward selects nothing: it runs the step without the guide launch)
    if (guide) FL_TRY(set_guide_ctl(m, c));
    const int kind = (lp ? kStepLp : 0) | (rules ? kStepRules : 0) | (guide ? kStepGuide : 0);
    if (T == 1) {
        FL_TRY(set_state(m, c, ids[0], pos, c->len, 0, -1, (size_t)-1, &sampler));
        FL_TRY(decode_step(m, c, (int64_t)c->len, kind));
        c->len += 1;
    } else {
        const int64_t chunk_max = tune(TK_PREFILL_CHUNK);
        size_t done = 0;
        const size_t call0 = c->len;                 // the mask of every chunk is that of the single call
        while (done < T) {
            int64_t Tc = (int64_t)std::min<size_t>(T - done, (size_t)chunk_max);
            if (T - done - (size_t)Tc == 1 && Tc > 2) Tc -= 1;      // never leave a 1-token tail (it would take the decode mask)
            for (auto &sh : m->shards) {
                FL_HIP(hipSetDevice(sh.device));
                if (sh.pre.cap_T < Tc) FL_TRY(grow_prefill_scratch(m, sh, Tc));
                FL_HIP(hipMemcpyAsync(sh.pre.ids, ids + done, (size_t)Tc * 4, hipMemcpyHostToDevice, sh.stream));
            }
            FL_TRY(set_state(m, c, ids[done], pos + done, c->len, 0, -1, call0, &sampler));
            if (Tc == 1) {
                // a 1-token tail chunk goes through the decode kernels but is still one `forward`
                FL_TRY(enqueue_forward(m, c, false, 1, false, (int64_t)c->len));
            } else {
                FL_TRY(enqueue_forward(m, c, true, Tc, true, (int64_t)c->len));
            }
            c->len += (size_t)Tc;
            done += (size_t)Tc;
        }
        FL_TRY(enqueue_argmax(m, c, 0, rules, guide));
        if (lp) FL_TRY(enqueue_logprobs(m, c, 0));
    }
    Shard &s0 = m->shards[0];
    FL_HIP(hipSetDevice(s0.device));
    if (logits_out) FL_HIP(hipMemcpyAsync(m->host_logits, s0.logits_full, (size_t)m->D.V * 4, hipMemcpyDeviceToHost, s0.stream));
    FL_TRY(finish_call(m, c, token_out ? 1 : 0, lp ? 1 : 0));
    if (logits_out) memcpy(logits_out, m->host_logits, (size_t)m->D.V * 4);
    if (token_out) *token_out = m->host_tokens[0];
    if (guide) c->guide_state = c->guide->walk(c->guide_state, m->host_tokens[0]);
    if (lp) scatter_logprobs(m->host_lp[0], lp, 0);
    return FL_OK;
}

int decode_greedy(Model *m, Cache *c, uint32_t first, size_t pos, size_t n_steps, int64_t eos,
                  uint32_t *tokens_out, size_t *n_out, const fl_sampler *sampling, const fl_logprobs *lp, float *last_row_out) {
    if (n_out) *n_out = 0;
    if (n_steps == 0) return FL_OK;
    FL_TRY(check_call(m, c, n_steps, pos));
    SampleState sampler;
    FL_TRY(make_sampler(sampling, m->D.V, &sampler));
    if (!tokens_out) FL_FAIL(FL_ERR_BAD_ARGUMENT, "null tokens_out");
    FL_TRY(check_token(m, first, "token"));
    if (lp) { FL_TRY(check_logprobs(lp, m->D.V)); FL_TRY(logprobs_supported(m)); }
    std::lock_guard<std::mutex> lock(m->mu);
    if (lp) { FL_TRY(ensure_logprobs(m, c)); FL_TRY(set_logprobs(m, c, lp)); }
    if (c->rules_on) FL_TRY(set_logit_rules_ctl(m, c, true));      // every step's input token is one more output
    const Guide *guide = c->guide;
    const int kind = (lp ? kStepLp : 0) | (c->rules_on ? kStepRules : 0) | (guide ? kStepGuide : 0);
    size_t done = 0;
    uint32_t tok = first;
    // With an EOS id the host looks at the tokens between chunks of 16, 32, ... 256 steps: the reference's loop breaks at
    // the first EOS (mod.rs:431-436), and a request that ends after 20 tokens must not pay for n_steps forwards.  Without
    // one, a chunk is as long as the token buffer allows (one sync per 4096 steps).
    size_t chunk = eos >= 0 ? 16 : kOutTokensCap;
    while (done < n_steps) {
        const size_t nb = std::min(n_steps - done, chunk);
        if (eos >= 0) chunk = std::min<size_t>(chunk * 2, 256);
        FL_TRY(set_state(m, c, tok, pos + done, c->len, 0, eos, (size_t)-1, done == 0 ? &sampler : nullptr));
        if (guide) FL_TRY(set_guide_ctl(m, c));                     // the host's state: the device advances it inside the chunk
        for (size_t i = 0; i < nb; i++) FL_TRY(decode_step(m, c, (int64_t)(c->len + i), kind));
        FL_TRY(finish_call(m, c, nb, lp ? nb : 0));
        // (the raw row of the last step that ran, while the model is still locked: nobody else's step can have replaced it)
        if (last_row_out) FL_HIP(hipMemcpy(last_row_out, m->shards[0].logits_full, (size_t)m->D.V * 4, hipMemcpyDeviceToHost));
        for (size_t i = 0; i < nb; i++) {
            const uint32_t t = m->host_tokens[i];
            if (guide) c->guide_state = guide->walk(c->guide_state, t);      // (the EOS's edge too; what ran behind it is discarded)
            if (eos >= 0 && (int64_t)t == eos) {
                // the forward that produced EOS was needed; what ran after it is discarded
                c->len += i + 1;
                if (n_out) *n_out = done + i;
                return FL_OK;
            }
            tokens_out[done + i] = t;
            if (lp) scatter_logprobs(m->host_lp[i], lp, done + i);
        }
        c->len += nb;
        tok = m->host_tokens[nb - 1];
        done += nb;
    }
    if (n_out) *n_out = done;
    return FL_OK;
}

// ------------------------------------------------------------------------------- prompt log-probabilities (fl_forward_score, fl_batch_score)
int check_score(const fl_score *sc, size_t T, int64_t V) {
    if (!sc) FL_FAIL(FL_ERR_BAD_ARGUMENT, "null fl_score (sc)");
    if (sc->struct_size != sizeof(fl_score)) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_score.struct_size is %u, expected %zu", sc->struct_size, sizeof(fl_score));
    if (sc->top_n < 0 || sc->top_n > FL_LOGPROBS_MAX_TOP) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_score.top_n %d not in 0..%d", sc->top_n, FL_LOGPROBS_MAX_TOP);
    if (!sc->target_logprob) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_score.target_logprob is null");
    if (sc->top_n > 0 && !sc->top_ids) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_score.top_ids is null with top_n %d", sc->top_n);
    if (sc->top_n > 0 && !sc->top_logprobs) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_score.top_logprobs is null with top_n %d", sc->top_n);
    if (sc->_reserved[0] || sc->_reserved[1]) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_score._reserved must be 0");
    if (V > 0 && sc->top_n > V) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_score.top_n %d exceeds the vocabulary %lld", sc->top_n, (long long)V);
    if (V > 0 && sc->targets)
        for (size_t t = 0; t < T; t++)
            if (sc->targets[t] != FL_SCORE_NO_TARGET && (int64_t)sc->targets[t] >= V)
                FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_score.targets[%zu] = %u out of range (vocab %lld)", t, sc->targets[t], (long long)V);
    return FL_OK;
}

static int score_supported(const Model *m) {
    if (m->tp > 1 || m->shards.size() != 1) FL_FAIL(FL_ERR_UNSUPPORTED, "prompt log-probabilities do not run under tensor parallelism (tp_size %d)", m->tp);
    return FL_OK;
}

static int score_block_rows() { return std::max(1, std::min(1024, tune(TK_SCORE_ROWS))); }

// (never inside a stream capture: the model is locked and scoring launches eagerly)
int score_block_scratch(Model *m, Shard &sh, float **rows, int64_t *R_out) {
    ScoreScratch &ss = sh.score;
    const int64_t R = score_block_rows(), V = m->D.V;
    if (ss.cap_R < R) {
        FL_HIP(hipStreamSynchronize(sh.stream));                                         // (idle anyway: every call ends with a synchronise)
        if (ss.rows) { (void)hipFree(ss.rows); ss.rows = nullptr; }
        m->hbm_bytes -= ss.cap_R * V * 4; ss.bytes -= ss.cap_R * V * 4; ss.cap_R = 0;
        std::vector<void *> own;
        FL_TRY(dev_alloc(own, (void **)&ss.rows, (size_t)(R * V) * 4, nullptr));
        m->hbm_bytes += R * V * 4; ss.bytes += R * V * 4; ss.cap_R = R;
    }
    if (rows) *rows = ss.rows;
    if (R_out) *R_out = R;
    return FL_OK;
}

int ScoreCall::begin(const uint32_t *tg) {
    ScoreScratch &ss = sh.score;
    FL_HIP(hipSetDevice(sh.device));
    FL_TRY(score_block_scratch(m, sh, nullptr, nullptr));
    if (ss.cap_T < T) {
        FL_HIP(hipStreamSynchronize(sh.stream));                                         // (idle anyway: every call ends with a synchronise)
        const size_t per = 4 + sizeof(ScoreRec);
        if (ss.targets) (void)hipFree(ss.targets);
        if (ss.recs) (void)hipFree(ss.recs);
        if (ss.host_targets) (void)hipHostFree(ss.host_targets);
        if (ss.host_recs) (void)hipHostFree(ss.host_recs);
        ss.targets = nullptr; ss.recs = nullptr; ss.host_targets = nullptr; ss.host_recs = nullptr;
        m->hbm_bytes -= (int64_t)(ss.cap_T * per); ss.bytes -= (int64_t)(ss.cap_T * per); ss.cap_T = 0;
        const size_t cap = std::max<size_t>(T + T / 2, 256);
        std::vector<void *> own;
        FL_TRY(dev_alloc(own, (void **)&ss.targets, cap * 4, nullptr));
        FL_TRY(dev_alloc(own, (void **)&ss.recs, cap * sizeof(ScoreRec), nullptr));
        FL_HIP(hipHostMalloc((void **)&ss.host_targets, cap * 4, hipHostMallocDefault));
        FL_HIP(hipHostMalloc((void **)&ss.host_recs, cap * sizeof(ScoreRec), hipHostMallocDefault));
        m->hbm_bytes += (int64_t)(cap * per); ss.bytes += (int64_t)(cap * per); ss.cap_T = cap;
    }
    memcpy(ss.host_targets, tg, T * 4);
    FL_HIP(hipMemcpyAsync(ss.targets, ss.host_targets, T * 4, hipMemcpyHostToDevice, sh.stream));
    return FL_OK;
}

int ScoreCall::one(Launcher &L, const float *row, size_t at) {
    ScoreScratch &ss = sh.score;
    FL_TRY(launch_score_rows(L, row, m->D.V, 1, ss.targets + at, sc->top_n, ss.recs + at));
    if (sc->logits_out) FL_HIP(hipMemcpyAsync(sc->logits_out + at * (size_t)m->D.V, row, (size_t)m->D.V * 4, hipMemcpyDeviceToHost, sh.stream));
    return FL_OK;
}

AllRows ScoreCall::sink(size_t row0) {
    ScoreScratch &ss = sh.score;
    ScoreCall self = *this;
    return AllRows{ss.rows, std::min<int64_t>(ss.cap_R, score_block_rows()), [self, row0](Launcher &L, int64_t r0, int64_t n) -> int {
        ScoreScratch &s2 = self.sh.score;
        const size_t at = row0 + (size_t)r0, V = (size_t)self.m->D.V;
        FL_TRY(launch_score_rows(L, s2.rows, (int64_t)V, (int)n, s2.targets + at, self.sc->top_n, s2.recs + at));
        // (the diagnostic copy: stream-ordered, so the next block's lm_head overwrites the rows only behind it)
        if (self.sc->logits_out) FL_HIP(hipMemcpyAsync(self.sc->logits_out + at * V, s2.rows, (size_t)n * V * 4, hipMemcpyDeviceToHost, self.sh.stream));
        return FL_OK;
    }};
}

int ScoreCall::fetch() {
    ScoreScratch &ss = sh.score;
    FL_HIP(hipMemcpyAsync(ss.host_recs, ss.recs, T * sizeof(ScoreRec), hipMemcpyDeviceToHost, sh.stream));
    return FL_OK;
}

void ScoreCall::end() {
    const ScoreRec *r = sh.score.host_recs;
    const size_t n = (size_t)sc->top_n;
    for (size_t t = 0; t < T; t++) {
        sc->target_logprob[t] = r[t].lp.chosen;
        if (sc->target_rank) sc->target_rank[t] = r[t].rank;
        for (size_t j = 0; j < n; j++) { sc->top_ids[t * n + j] = r[t].lp.ids[j]; sc->top_logprobs[t * n + j] = r[t].lp.lps[j]; }
    }
}

// fl_forward with every row scored: the same chunks, the same mask, the same per-layer launches; behind each chunk's layers the final
// norm runs on all its rows and lm_head in blocks of score_rows rows, each followed by one score_rows launch.  Nothing is selected,
// and a cache's logit rules or guide are neither applied nor counted: the distribution is the model's own.
int forward_score(Model *m, Cache *c, const uint32_t *ids, size_t T, size_t pos, const fl_score *sc) {
    FL_TRY(check_score(sc, T, 0));
    FL_TRY(check_call(m, c, T, pos));
    debug_inject("forward");
    if (!ids) FL_FAIL(FL_ERR_BAD_ARGUMENT, "null ids");
    for (size_t t = 0; t < T; t++) FL_TRY(check_token(m, ids[t], "token"));
    FL_TRY(check_score(sc, T, m->D.V));
    FL_TRY(score_supported(m));
    std::vector<uint32_t> tg(T, kScoreNoTarget);
    for (size_t t = 0; t < T; t++) if (sc->targets ? true : t + 1 < T) tg[t] = sc->targets ? sc->targets[t] : ids[t + 1];
    std::lock_guard<std::mutex> lock(m->mu);
    Shard &sh = m->shards[0];
    ScoreCall call{m, sh, sc, T};
    FL_TRY(call.begin(tg.data()));
    const SampleState argmax{};
    if (T == 1) {
        // the decode step's forward (its mask, its kernels); the row is the one it leaves in logits_full
        FL_TRY(set_state(m, c, ids[0], pos, c->len, 0, -1, (size_t)-1, &argmax));
        FL_TRY(enqueue_forward(m, c, false, 1, false, (int64_t)c->len));
        Launcher L = make_launcher(m, sh);
        FL_TRY(call.one(L, sh.logits_full, 0));
        c->len += 1;
    } else {
        const int64_t chunk_max = tune(TK_PREFILL_CHUNK);
        size_t done = 0;
        const size_t call0 = c->len;                 // the mask of every chunk is that of the single call
        while (done < T) {
            int64_t Tc = (int64_t)std::min<size_t>(T - done, (size_t)chunk_max);
            if (T - done - (size_t)Tc == 1 && Tc > 2) Tc -= 1;      // never leave a 1-token tail (it would take the decode mask)
            FL_HIP(hipSetDevice(sh.device));
            if (sh.pre.cap_T < Tc) FL_TRY(grow_prefill_scratch(m, sh, Tc));
            FL_HIP(hipMemcpyAsync(sh.pre.ids, ids + done, (size_t)Tc * 4, hipMemcpyHostToDevice, sh.stream));
            FL_TRY(set_state(m, c, ids[done], pos + done, c->len, 0, -1, call0, &argmax));
            if (Tc == 1) {
                FL_TRY(enqueue_forward(m, c, false, 1, false, (int64_t)c->len));
                Launcher L = make_launcher(m, sh);
                FL_TRY(call.one(L, sh.logits_full, done));
            } else {
                const AllRows rows = call.sink(done);
                FL_TRY(enqueue_forward(m, c, true, Tc, true, (int64_t)c->len, &rows));
            }
            c->len += (size_t)Tc;
            done += (size_t)Tc;
        }
    }
    FL_TRY(call.fetch());
    FL_TRY(finish_call(m, c, 0));
    call.end();
    return FL_OK;
}

// ------------------------------------------------------------------------------- speculative greedy decode
int cache_truncate(Cache *c, size_t len) {
    if (!c) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_cache_truncate: null cache");
    if (len > c->len) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_cache_truncate: %zu is beyond the cached length %zu", len, c->len);
    c->len = len;                                // (the device StepState is written from this at the start of every call)
    return FL_OK;
}

// ------------------------------------------------------------------------------- prefix reuse across caches
// fl_cache_copy_prefix: dst takes the first n cached positions of src.  Two caches of one model differ only in seq_alloc, so per
// shard the prefix of K (and of a row-major V) is L * Hkvs rows of n * d * es bytes at pitch seq_alloc * d * es, and the prefix of a
// transposed V is L * Hkvs * d rows of n * es bytes at pitch seq_alloc * es: one launch of k_kvcopy.hip per shard, on the shard's
// stream and under the model mutex, i.e. behind everything already submitted for either cache and before anything submitted later.
// Not waited for: ~Cache synchronises every shard's stream under the same mutex before it frees, so src cannot go away under the copy.
// The length is host state, as in cache_truncate; dst's graph, split counts and layout choices stay as its capacity made them.
int cache_copy_prefix(Cache *dst, const Cache *src, size_t n) {
    if (!dst || !src) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_cache_copy_prefix: null cache");
    if (dst->m != src->m) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_cache_copy_prefix: the caches belong to different models");
    if (src == dst) return cache_truncate(dst, n);
    if (n > src->len) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_cache_copy_prefix: %zu is beyond the source's cached length %zu", n, src->len);
    if (n > dst->max_seq) FL_FAIL(FL_ERR_SEQ_OVERFLOW, "fl_cache_copy_prefix: %zu positions exceed the destination's capacity %zu", n, dst->max_seq);
    if (n == 0) { dst->len = 0; return FL_OK; }
    if (dst->v_transposed != src->v_transposed)
        FL_FAIL(FL_ERR_UNSUPPORTED, "fl_cache_copy_prefix: the caches keep V in different layouts (the attention switch changed between their creation)");
    Model *m = dst->m;
    debug_inject("cache_copy_prefix");
    std::lock_guard<std::mutex> lock(m->mu);
    const int64_t es = (int64_t)m->esize(), d = m->D.d;
    for (size_t i = 0; i < m->shards.size(); i++) {
        Shard &sh = m->shards[i];
        FL_HIP(hipSetDevice(sh.device));
        const int64_t heads = m->D.L * sh.Hkvs;
        KvCopyJob k, v;
        k.src = src->shards[i].k; k.dst = dst->shards[i].k;
        k.rows = heads; k.width = (int64_t)n * d * es;
        k.spitch = (int64_t)src->seq_alloc * d * es; k.dpitch = (int64_t)dst->seq_alloc * d * es;
        v = k;
        v.src = src->shards[i].v; v.dst = dst->shards[i].v;
        if (dst->v_transposed) {
            v.rows = heads * d; v.width = (int64_t)n * es;
            v.spitch = (int64_t)src->seq_alloc * es; v.dpitch = (int64_t)dst->seq_alloc * es;
        }
        Launcher L = make_launcher(m, sh);
        FL_TRY(launch_kv_copy(L, k, v));
    }
    dst->len = n;
    return FL_OK;
}

int check_lookup(const fl_lookup *o) {
    if (!o) FL_FAIL(FL_ERR_BAD_ARGUMENT, "null fl_lookup");
    if (o->struct_size != sizeof(fl_lookup)) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_lookup.struct_size is %u, expected %zu", o->struct_size, sizeof(fl_lookup));
    if (o->max_draft < 0 || o->max_draft > FL_VERIFY_MAX_DRAFT) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_lookup.max_draft %d outside 0 .. %d", o->max_draft, FL_VERIFY_MAX_DRAFT);
    if (o->ngram_min < 1 || o->ngram_min > o->ngram_max || o->ngram_max > kLookupMaxNgram)
        FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_lookup: need 1 <= ngram_min <= ngram_max <= %d (got %d, %d)", kLookupMaxNgram, o->ngram_min, o->ngram_max);
    return FL_OK;
}

// what a verify step may and may not be asked: everything here is decided before the device is touched
int check_verify(Model *m, Cache *c, size_t n_draft, size_t pos) {
    if (n_draft > FL_VERIFY_MAX_DRAFT) FL_FAIL(FL_ERR_BAD_ARGUMENT, "n_draft %zu exceeds FL_VERIFY_MAX_DRAFT (%d)", n_draft, FL_VERIFY_MAX_DRAFT);
    FL_TRY(check_call(m, c, n_draft + 1, pos));
    if (n_draft > 0 && m->tp > 1) FL_FAIL(FL_ERR_UNSUPPORTED, "the verify step does not run under tensor parallelism (tp_size %d)", m->tp);
    if (m->D.window >= 0 && (int64_t)n_draft > m->D.window)
        FL_FAIL(FL_ERR_UNSUPPORTED, "n_draft %zu exceeds sliding_window %lld: the rows would no longer equal successive decode steps", n_draft, (long long)m->D.window);
    return FL_OK;
}

// one verify step with the model locked and the arguments checked; host_verify holds the ids and the accepted count afterwards.
// sampler (null or on == 0: ArgMax, the launches there have always been): row i is drawn with word sampler->draw + i, and the host
// stays authoritative for the draw count as it is for the cache length -- every call brings the state, nothing is left behind.
// adjust (fl_forward_verify_lp / fl_decode_lookup_lp only; the other callers have refused such caches): the cache's logit rules and
// guide are applied by ONE launch in front of the selection, which then reads the adjusted rows -- row i with the table as it stands
// after the inputs of rows 0..i and in the guide state after drafts 0..i-1; the table and c->guide_state are left as they were, for
// verify_commit once the caller knows which rows count.  lp: the RAW rows are scored against the ids the selection left on the device.
// Without rules, guide and lp the launches are the ones above, unchanged.
static int verify_step(Model *m, Cache *c, uint32_t token, const uint32_t *draft, size_t n_draft, size_t pos, float *logits_out,
                       const SampleState *sampler = nullptr, bool adjust = false, const fl_logprobs *lp = nullptr) {
    const Dims &D = m->D;
    Shard &sh = m->shards[0];
    const int64_t T = (int64_t)n_draft + 1;
    const bool rules = adjust && c->rules_on;
    const Guide *guide = adjust ? c->guide : nullptr;
    FL_HIP(hipSetDevice(sh.device));
    if (!sh.verify_logits) {
        FL_TRY(dev_alloc(sh.allocs, (void **)&sh.verify_out, kVerifyWords * 4, &m->hbm_bytes));
        FL_HIP(hipMemsetAsync(sh.verify_out, 0, kVerifyWords * 4, sh.stream));
        FL_HIP(hipHostMalloc((void **)&m->host_verify, kVerifyWords * 4, hipHostMallocDefault));
        FL_TRY(dev_alloc(sh.allocs, (void **)&sh.verify_logits, (size_t)kVerifyMaxRows * D.V * 4, &m->hbm_bytes));
    }
    const bool sampled = sampler && sampler->on;
    if (sampled && !sh.verify_scratch) FL_TRY(dev_alloc(sh.allocs, (void **)&sh.verify_scratch, (size_t)kVerifyMaxRows * D.V * 4, &m->hbm_bytes));
    if ((rules || guide) && !sh.verify_adjusted) FL_TRY(dev_alloc(sh.allocs, (void **)&sh.verify_adjusted, (size_t)kVerifyMaxRows * D.V * 4, &m->hbm_bytes));
    if (lp && !sh.verify_recs) {
        FL_TRY(dev_alloc(sh.allocs, (void **)&sh.verify_recs, kVerifyMaxRows * sizeof(ScoreRec), &m->hbm_bytes));
        if (!m->host_verify_recs) FL_HIP(hipHostMalloc((void **)&m->host_verify_recs, kVerifyMaxRows * sizeof(ScoreRec), hipHostMallocDefault));
    }
    if (sh.pre.cap_T < T) FL_TRY(grow_prefill_scratch(m, sh, T));
    uint32_t *ids = m->host_tokens;                                  // pinned, and idle until this call's sync
    ids[0] = token;
    for (size_t i = 0; i < n_draft; i++) ids[1 + i] = draft[i];
    FL_HIP(hipMemcpyAsync(sh.pre.ids, ids, (size_t)T * 4, hipMemcpyHostToDevice, sh.stream));
    const SampleState argmax{};
    FL_TRY(set_state(m, c, token, pos, c->len, 0, -1, c->len, &argmax));
    const AllRows rows{sh.verify_logits, T, nullptr};
    FL_TRY(enqueue_forward(m, c, true, T, true, (int64_t)c->len, &rows));
    Launcher L = make_launcher(m, sh);
    const float *sel = sh.verify_logits;                             // what the selection reads
    if (rules || guide) {
        VerifyAdjustArgs a;
        for (int64_t i = 0; i < T; i++) a.ids[i] = ids[i];
        if (rules) { a.table = c->shards[0].rule_tab; a.rp = c->rule_rp; a.fp = c->rule_fp; a.pp = c->rule_pp; }
        if (guide) {
            a.row_ptr = guide->row_ptr_dev; a.tokens = guide->tokens_dev;
            uint32_t s = c->guide_state;
            for (int64_t i = 0; i < T; i++) { a.states[i] = s; if (i < (int64_t)n_draft) s = guide->walk(s, draft[i]); }
        }
        a.out = sh.verify_adjusted;
        FL_TRY(launch_verify_adjust(L, sh.verify_logits, D.V, (int)T, a));
        sel = sh.verify_adjusted;
    }
    if (sampled) FL_TRY(launch_verify_sample(L, sel, D.V, (int)T, sh.pre.ids + 1, *sampler, sh.verify_scratch, sh.verify_out, nullptr));
    else FL_TRY(launch_verify_select(L, sel, D.V, (int)T, sh.pre.ids + 1, sh.verify_out));
    if (lp) {                                                        // the model's own distribution: the raw rows, the selected ids as targets
        FL_TRY(launch_score_rows(L, sh.verify_logits, D.V, (int)T, sh.verify_out, lp->top_n, sh.verify_recs));
        FL_HIP(hipMemcpyAsync(m->host_verify_recs, sh.verify_recs, (size_t)T * sizeof(ScoreRec), hipMemcpyDeviceToHost, sh.stream));
    }
    FL_HIP(hipMemcpyAsync(m->host_verify, sh.verify_out, (kVerifyNacc + 1) * 4, hipMemcpyDeviceToHost, sh.stream));
    FL_TRY(finish_call(m, c, 0));
    if (m->host_verify[kVerifyNacc] > n_draft) FL_FAIL(FL_ERR_HIP, "verify step: accepted count %u out of range", m->host_verify[kVerifyNacc]);
    if (logits_out) FL_HIP(hipMemcpy(logits_out, sh.verify_logits, (size_t)T * D.V * 4, hipMemcpyDeviceToHost));
    c->len += (size_t)m->host_verify[kVerifyNacc] + 1;               // rejected rows' K/V stay behind the length; the next append overwrites them
    return FL_OK;
}

// ------------------------------------------------------------------------------- verify steps with rules, a guide and log-probs
// true, and *next: the state has an edge for t (Guide::walk cannot tell "no edge" from an edge back to the same state)
static bool guide_edge(const Guide *g, uint32_t s, uint32_t t, uint32_t *next) {
    const uint32_t *b = g->tokens.data() + g->row_ptr[s], *e = g->tokens.data() + g->row_ptr[s + 1];
    const uint32_t *it = std::lower_bound(b, e, t);
    if (it == e || *it != t) return false;
    *next = g->next[(size_t)(it - g->tokens.data())];
    return true;
}

// A draft id without an edge from the state reached is -inf in the row before it and can never be accepted: the draft ends there.
static size_t guide_cut_draft(const Cache *c, const uint32_t *draft, size_t n_draft) {
    if (!c->guide) return n_draft;
    uint32_t s = c->guide_state;
    for (size_t i = 0; i < n_draft; i++) if (!guide_edge(c->guide, s, draft[i], &s)) return i;
    return n_draft;
}

// What a ruled / guided verify step leaves behind, once the caller knows which rows count (the model locked, behind verify_step): the
// inputs of rows 0 .. n_rows-1 -- token, draft[0 .. n_rows-1) -- are counted into the rules table by one launch on the shard's stream,
// behind the selection and ahead of everything submitted later; the ids the call returns (an EOS that ended it included) move the guide.
static int verify_commit(Model *m, Cache *c, uint32_t token, const uint32_t *draft, size_t n_rows, const uint32_t *ret, size_t n_ret) {
    if (c->rules_on && n_rows > 0) {
        Shard &sh = m->shards[0];
        FL_HIP(hipSetDevice(sh.device));
        RulesCountArgs a;
        a.n = (int)n_rows;
        a.ids[0] = token;
        for (size_t i = 1; i < n_rows; i++) a.ids[i] = draft[i - 1];
        Launcher L = make_launcher(m, sh);
        FL_TRY(launch_rules_count(L, c->shards[0].rule_tab, m->D.V, a));
    }
    if (c->guide) for (size_t i = 0; i < n_ret; i++) c->guide_state = c->guide->walk(c->guide_state, ret[i]);
    return FL_OK;
}

// lp's arrays from entry `at` on
static fl_logprobs logprobs_from(const fl_logprobs *lp, size_t at) {
    fl_logprobs r = *lp;
    r.token_logprob += at;
    if (r.top_ids) r.top_ids += at * (size_t)lp->top_n;
    if (r.top_logprobs) r.top_logprobs += at * (size_t)lp->top_n;
    return r;
}

// one counted, guided step of the plain loop (fl_decode_sample_lp with n_steps 1): what a verify call without drafts is, bit for bit.
// logits_out: the step's raw row, copied while decode_greedy still holds the model's lock.
static int plain_step(Model *m, Cache *c, uint32_t token, size_t pos, const fl_sampler *sampling, const fl_logprobs *lp, uint32_t *token_out,
                      float *logits_out) {
    size_t n = 0;
    return decode_greedy(m, c, token, pos, 1, -1, token_out, &n, sampling, lp, logits_out);
}

// fl_forward_verify{,_ex} (full == false: a cache with rules or a guide is refused, lp is null) and fl_forward_verify_lp (full: the
// superset).  One body, so the two cannot drift apart; `who` names the entry point in the messages.
static int verify_call(Model *m, Cache *c, uint32_t token, const uint32_t *draft, size_t n_draft, size_t pos, const fl_sampler *sampling,
                       const fl_logprobs *lp, uint32_t *tokens_out, size_t *n_out, float *logits_out, bool full, const char *who) {
    if (n_out) *n_out = 0;
    SampleState sampler;
    FL_TRY(make_sampler(sampling, 0, &sampler));                     // its argument errors, before the handles are looked at
    if (lp) FL_TRY(check_logprobs(lp, 0));
    if (!tokens_out || !n_out) FL_FAIL(FL_ERR_BAD_ARGUMENT, "%s: null tokens_out or n_out", who);
    if (n_draft > 0 && !draft) FL_FAIL(FL_ERR_BAD_ARGUMENT, "%s: null draft", who);
    if (!full) { FL_TRY(refuse_logit_rules(c, who)); FL_TRY(refuse_guide(c, who)); }
    FL_TRY(check_verify(m, c, n_draft, pos));
    FL_TRY(check_token(m, token, "token"));
    for (size_t i = 0; i < n_draft; i++) FL_TRY(check_token(m, draft[i], "draft"));
    if (lp) { FL_TRY(check_logprobs(lp, m->D.V)); FL_TRY(logprobs_supported(m)); }
    if (full) n_draft = guide_cut_draft(c, draft, n_draft);
    if (n_draft == 0) {
        // the decode step itself: its mask, its kernels.  A ruled or guided cache, or one asked for log-probs, takes the COUNTED step of
        // the plain loop; a bare one the step it has always taken (fl_forward_sample_ex of one token: rules would not be counted there)
        if (full && (c->rules_on || c->guide || lp)) FL_TRY(plain_step(m, c, token, pos, sampler.on ? sampling : nullptr, lp, tokens_out, logits_out));
        else FL_TRY(forward(m, c, &token, 1, pos, logits_out, tokens_out, sampler.on ? sampling : nullptr));
        *n_out = 1;
        return FL_OK;
    }
    FL_TRY(make_sampler(sampling, m->D.V, &sampler));                // (with the vocabulary: a top_k >= V is off)
    debug_inject("forward");
    std::lock_guard<std::mutex> lock(m->mu);
    FL_TRY(verify_step(m, c, token, draft, n_draft, pos, logits_out, &sampler, full, lp));
    const size_t n = (size_t)m->host_verify[kVerifyNacc] + 1;
    if (full) FL_TRY(verify_commit(m, c, token, draft, n, m->host_verify, n));
    for (size_t i = 0; i < n; i++) {
        tokens_out[i] = m->host_verify[i];
        if (lp) scatter_logprobs(m->host_verify_recs[i].lp, lp, i);
    }
    *n_out = n;
    return FL_OK;
}

int forward_verify(Model *m, Cache *c, uint32_t token, const uint32_t *draft, size_t n_draft, size_t pos, uint32_t *tokens_out,
                   size_t *n_out, float *logits_out, const fl_sampler *sampling) {
    return verify_call(m, c, token, draft, n_draft, pos, sampling, nullptr, tokens_out, n_out, logits_out, false, "fl_forward_verify");
}

int forward_verify_lp(Model *m, Cache *c, uint32_t token, const uint32_t *draft, size_t n_draft, size_t pos, const fl_sampler *sampling,
                      const fl_logprobs *lp, uint32_t *tokens_out, size_t *n_out, float *logits_out) {
    return verify_call(m, c, token, draft, n_draft, pos, sampling, lp, tokens_out, n_out, logits_out, true, "fl_forward_verify_lp");
}

// fl_decode_lookup{,_ex} (full == false) and fl_decode_lookup_lp (full): one loop.
static int lookup_loop(Model *m, Cache *c, const uint32_t *corpus, size_t n_corpus, uint32_t first, size_t pos, size_t n_steps, int64_t eos,
                       const fl_lookup *opts, const fl_sampler *sampling, const fl_logprobs *lp, uint32_t *tokens_out, size_t *n_out,
                       fl_spec_stats *stats, bool full, const char *who) {
    if (n_out) *n_out = 0;
    if (stats) *stats = fl_spec_stats{};
    FL_TRY(check_lookup(opts));
    SampleState sampler;
    FL_TRY(make_sampler(sampling, 0, &sampler));                     // its argument errors, before the handles are looked at
    const bool sampled = sampler.on != 0;                            // false: the greedy loop, launch for launch
    if (lp) FL_TRY(check_logprobs(lp, 0));
    if (!n_out) FL_FAIL(FL_ERR_BAD_ARGUMENT, "%s: null n_out", who);
    if (n_corpus && !corpus) FL_FAIL(FL_ERR_BAD_ARGUMENT, "%s: null corpus", who);
    if (!full) { FL_TRY(refuse_logit_rules(c, who)); FL_TRY(refuse_guide(c, who)); }
    if (n_steps == 0) return FL_OK;
    if (!tokens_out) FL_FAIL(FL_ERR_BAD_ARGUMENT, "%s: null tokens_out", who);
    FL_TRY(check_call(m, c, n_steps, pos));
    FL_TRY(check_token(m, first, "token"));
    if (m->tp > 1 && opts->max_draft > 0) FL_FAIL(FL_ERR_UNSUPPORTED, "the verify step does not run under tensor parallelism (tp_size %d)", m->tp);
    if (lp) { FL_TRY(check_logprobs(lp, m->D.V)); FL_TRY(logprobs_supported(m)); }
    const size_t V = (size_t)m->D.V, L0 = c->len;
    // a cache with rules or a guide, or a call that wants log-probs, takes the plain loop's COUNTED step where nothing is drafted; a
    // bare one the steps fl_decode_lookup{,_ex} have always taken
    const bool counted = full && (c->rules_on || c->guide || lp);
    if (opts->max_draft == 0 && (sampled || counted)) {              // nothing to verify: the plain loop itself
        FL_TRY(decode_greedy(m, c, first, pos, n_steps, eos, tokens_out, n_out, sampled ? sampling : nullptr, lp));
        if (stats) stats->steps = c->len - L0;
        return FL_OK;
    }
    std::vector<uint32_t> hist;
    hist.reserve(n_corpus + 1 + n_steps + FL_VERIFY_MAX_DRAFT + 1);
    for (size_t i = 0; i < n_corpus; i++) hist.push_back(corpus[i]);
    hist.push_back(first);
    uint32_t draft[FL_VERIFY_MAX_DRAFT + 1], got[FL_VERIFY_MAX_DRAFT + 1];
    uint32_t tok = first;
    size_t emitted = 0;
    while (emitted < n_steps) {
        // room: this step caches `tok` and up to n_draft drafts, and every later token still needs its own position
        size_t limit = n_steps - emitted - 1;
        limit = std::min(limit, c->max_seq - c->len - 1);
        limit = std::min(limit, (size_t)m->D.max_pos - (pos + emitted) - 1);
        if (m->D.window >= 0) limit = std::min(limit, (size_t)m->D.window);
        size_t nd = lookup_draft(hist.data(), hist.size(), opts->max_draft, opts->ngram_max, opts->ngram_min, limit, draft);
        for (size_t i = 0; i < nd; i++) if (draft[i] >= V) { nd = i; break; }      // (a corpus id the model does not have ends the draft)
        if (full) nd = guide_cut_draft(c, draft, nd);                // ... and so does one the guide cannot reach
        // token k of the request is drawn with word k, and reported in entry k of lp's arrays, whatever was rejected before
        fl_sampler sp{};
        if (sampled) { sp = *sampling; sp.draws_done += emitted; }
        fl_logprobs lps{};
        if (lp) lps = logprobs_from(lp, emitted);
        size_t n = 0, keep = 0;                                      // ids the step returned; how many of them are emitted
        if (nd == 0) {
            if (counted) FL_TRY(plain_step(m, c, tok, pos + emitted, sampled ? &sp : nullptr, lp ? &lps : nullptr, got, nullptr));
            else FL_TRY(forward(m, c, &tok, 1, pos + emitted, nullptr, got, sampled ? &sp : nullptr));
            n = 1;
            keep = eos >= 0 && (int64_t)got[0] == eos ? 0 : 1;
        } else {
            if (sampled) FL_TRY(make_sampler(&sp, m->D.V, &sampler));
            std::lock_guard<std::mutex> lock(m->mu);
            FL_TRY(verify_step(m, c, tok, draft, nd, pos + emitted, nullptr, &sampler, full, lp));
            n = (size_t)m->host_verify[kVerifyNacc] + 1;
            for (size_t i = 0; i < n; i++) got[i] = m->host_verify[i];
            keep = n;
            for (size_t i = 0; i < n; i++) if (eos >= 0 && (int64_t)got[i] == eos) { keep = i; break; }
            // an EOS at got[i]: rows 0..i were the plain loop's steps -- their inputs are counted, the EOS's edge is walked -- the rest is dropped
            const size_t rows = std::min(keep + 1, n);
            if (full) FL_TRY(verify_commit(m, c, tok, draft, rows, got, rows));
            if (lp) for (size_t i = 0; i < keep; i++) scatter_logprobs(m->host_verify_recs[i].lp, &lps, i);
        }
        if (stats) { stats->steps += 1; stats->drafted += nd; stats->accepted += n - 1; }
        for (size_t i = 0; i < keep; i++) {
            tokens_out[emitted++] = got[i];
            hist.push_back(got[i]);
        }
        if (keep < n) {
            // the forward that produced EOS was needed; what was accepted after it is dropped (fl_decode_greedy's length)
            c->len = L0 + emitted + 1;
            *n_out = emitted;
            return FL_OK;
        }
        tok = got[n - 1];
    }
    *n_out = emitted;
    return FL_OK;
}

int decode_lookup(Model *m, Cache *c, const uint32_t *corpus, size_t n_corpus, uint32_t first, size_t pos, size_t n_steps, int64_t eos,
                  const fl_lookup *opts, uint32_t *tokens_out, size_t *n_out, fl_spec_stats *stats, const fl_sampler *sampling) {
    return lookup_loop(m, c, corpus, n_corpus, first, pos, n_steps, eos, opts, sampling, nullptr, tokens_out, n_out, stats, false, "fl_decode_lookup");
}

int decode_lookup_lp(Model *m, Cache *c, const uint32_t *corpus, size_t n_corpus, uint32_t first, size_t pos, size_t n_steps, int64_t eos,
                     const fl_lookup *opts, const fl_sampler *sampling, const fl_logprobs *lp, uint32_t *tokens_out, size_t *n_out,
                     fl_spec_stats *stats) {
    return lookup_loop(m, c, corpus, n_corpus, first, pos, n_steps, eos, opts, sampling, lp, tokens_out, n_out, stats, true, "fl_decode_lookup_lp");
}

}  // namespace fl
